"""The three loss kernels of csrc/loss.hip at the shapes and values where their loops and branches change behaviour, against plain
float64 references on the CPU.  Needs a real MI355X.

tests/test_loss_gpu.py pins the kernels to three recorded fixtures with K <= 64, where no lane of a 64-strided reduction takes a second
trip.  Here: K from 1 to 513, masks without / with only positives, descriptor columns of norm 3 (exponents in the hundreds: only the
max-subtraction keeps them finite, softplus takes its `> 20` branch), saturated scores, zero patch pixels and zero descriptors, C that
is no multiple of the four channel groups, and the C ABI with row strides wider than K / C.

References.  desc_loss and fine_circle_loss: oracle/loss_oracle.py (pinned to the reference's model/loss.py by
tests/test_oracle_golden.py) in float64 with float64 torch.autograd.  overlap_loss: float64 torch.nn.BCELoss, which the reference calls
and whose backward, (x - y) / max((1 - x) x, 1e-12) / n, the kernel restates - the oracle's clamped-log expression has NaN gradients
at scores of exactly 0 and 1.  The inputs are created in float32 and upcast: both sides see the same numbers.

Tolerance.  Every tensor is judged norm-wise, |got - ref| / |ref|, scalars relatively, against TOL = 2e-5: the figure of
tests/test_loss_gpu.py for "fp32 sums in another order".  A dropped term or a skipped second loop trip is wrong by orders of magnitude
more.  Two exceptions, both reasoned from the mathematics and not from the kernel's output:
  * entries that are huge by construction (the gradients at saturated scores, up to 9e10, and at zero vectors, 1e5 ... 1e8) are compared
    on their own, so that they cannot drown the rest of their tensor;
  * with C = 1 the cosine of two scalars is +-1 and its gradient is analytically zero: the float64 reference is 0 up to its own
    cancellation, and a norm-wise ratio against it means nothing.  There the gradients are bounded in absolute value by TOL times the
    size of the terms that cancel (see `_circle_c1_allowance`).

Headroom.  Worst error over the cases of this file, norm-wise against the float64 reference (the saturated overlap gradients entry-wise):
the float32 oracle (the same expressions evaluated by torch in float32 on the CPU) on the same inputs, and the kernel.  Every test
prints both figures per tensor (pytest -rA); these are the largest of them, measured on an MI355X, with the tensor they come from.

    loss              float32 oracle                                    kernel
    desc_loss         2.6e-06  (K70_C16_norm3, d pc)                    2.6e-06  (K70_C16_norm3, d pc)
    overlap_loss      1.3e-07  ((31, 32), d outline)                    1.3e-07  ((700, 300), loss)
    fine_circle_loss  7.2e-07  (K6_C13_zero_negative_pixel, d patches)  2.1e-07  (K7_C13_zero_descriptor, d patches)

TOL leaves a factor of 8 on desc_loss's worst case and 90 or more on the other two losses; the kernels are no further from float64 than torch's own
float32 evaluation is.

Mutation check.  A 64-lane stride changed to 128 fails: in desc_lse_kernel's sum and in desc_final_kernel, the desc_loss cases K65,
K130, K200, K513 and K70; in mean_kernel, the circle cases K65_C64 and K200_C12; in bce_kernel, the overlap cases (33, 32) and
(700, 300).  The cases with K (or n_in + n_out) <= 64 pass under all four, as they must.
"""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_oracle as LO  # noqa: E402

DEV = "cuda:0"
TOL = 2e-5   # tests/test_loss_gpu.py: fp32 sums in another order than torch's
UP = 0.37    # a non-unit upstream gradient

COFI_EINVAL, COFI_EWORKSPACE = -1, -2


def gen(seed):
    return torch.Generator().manual_seed(seed)


def err(got, ref):
    """norm-wise relative error against the float64 reference (relative error for a scalar)"""
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    assert got.shape == ref.shape and torch.isfinite(got).all() and torch.isfinite(ref).all()
    d, n = float((got - ref).norm()), float(ref.norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


def report(what, case, name, e_kernel, e_f32):
    print("%s %s %s: kernel %.2e, float32 oracle %.2e" % (what, case, name, e_kernel, e_f32))


# ---------------------------------------------------------------------------------------------------------------------- desc_loss
def _unit_cols(C, K, g):
    return torch.nn.functional.normalize(torch.randn(C, K, generator=g), dim=0)


DESC_CASES = ["K1_C8_eye", "K63_C20_ragged", "K65_C128_eye", "K130_C20_no_positive", "K200_C64_all_positive", "K513_C32_eye",
              "K70_C16_norm3"]


def _desc_inputs(case):
    """-> img, pc (C, K), mask (K, K), float32 on the CPU"""
    g = gen(100 + DESC_CASES.index(case))
    if case == "K1_C8_eye":
        return _unit_cols(8, 1, g), _unit_cols(8, 1, g), torch.eye(1)
    if case == "K63_C20_ragged":   # a few off-diagonal positives, two rows without a positive
        mask = torch.eye(63)
        mask[3, 7] = mask[10, 2] = mask[40, 41] = mask[61, 0] = 1.0
        mask[5, :] = 0.0
        mask[62, :] = 0.0
        return _unit_cols(20, 63, g), _unit_cols(20, 63, g), mask
    if case == "K65_C128_eye":
        return _unit_cols(128, 65, g), _unit_cols(128, 65, g), torch.eye(65)
    if case == "K130_C20_no_positive":
        return _unit_cols(20, 130, g), _unit_cols(20, 130, g), torch.zeros(130, 130)
    if case == "K200_C64_all_positive":   # pc correlated to img: small distances on the diagonal
        img = _unit_cols(64, 200, g)
        pc = torch.nn.functional.normalize(img + 0.3 * torch.randn(64, 200, generator=g), dim=0)
        return img, pc, torch.ones(200, 200)
    if case == "K513_C32_eye":
        return _unit_cols(32, 513, g), _unit_cols(32, 513, g), torch.eye(513)
    if case == "K70_C16_norm3":   # <img_i, pc_j> up to +-9: exponents s (d - margin)^2 in the hundreds
        return 3.0 * _unit_cols(16, 70, g), 3.0 * _unit_cols(16, 70, g), torch.eye(70)
    raise KeyError(case)


DESC_HP = dict(pos_margin=0.2, neg_margin=1.8, log_scale=10.0)


def _oracle_desc(img, pc, mask):
    img, pc = img.clone().requires_grad_(), pc.clone().requires_grad_()
    loss, dists = LO.desc_loss(img, pc, mask, **DESC_HP)
    (UP * loss).backward()
    return dict(loss=loss.detach(), dists=dists.detach(), gimg=img.grad, gpc=pc.grad)


@functools.lru_cache(maxsize=None)
def desc_ref(case):
    """inputs, the float64 oracle's results and the float32 oracle's own error against them - computed once per case"""
    img, pc, mask = _desc_inputs(case)
    r64 = _oracle_desc(img.double(), pc.double(), mask.double())
    r32 = _oracle_desc(img, pc, mask)
    assert all(torch.isfinite(v).all() for v in list(r64.values()) + list(r32.values())), "the oracle itself must be finite on " + case
    return (img, pc, mask), r64, {k: err(r32[k], r64[k]) for k in r64}


def _run_desc(img, pc, mask):
    from cofii2p_amd.loss import desc_loss

    a, b = img.to(DEV).requires_grad_(), pc.to(DEV).requires_grad_()
    loss, dists = desc_loss(DEV, a, b, mask.to(DEV), **DESC_HP)
    (UP * loss).backward()
    return dict(loss=loss.detach(), dists=dists.detach(), gimg=a.grad, gpc=b.grad)


@pytest.mark.parametrize("case", DESC_CASES)
def test_desc_loss_against_float64_oracle(case):
    """loss, dists, d img, d pc (non-unit upstream gradient) within TOL of the float64 oracle; a second call gives the same bits
    (csrc/loss.hip: every reduction has a fixed order)"""
    (img, pc, mask), ref, e32 = desc_ref(case)
    got = _run_desc(img, pc, mask)
    errs = {k: err(got[k], ref[k]) for k in ref}
    for k in ref:
        report("desc_loss", case, k, errs[k], e32[k])
    for k in ref:
        assert errs[k] <= TOL, (case, k, errs[k])
    again = _run_desc(img, pc, mask)
    for k in ref:
        assert torch.equal(got[k], again[k]), (case, k)


def test_desc_loss_norm3_case_needs_the_max_subtraction():
    """the premise of the K70_C16_norm3 case, checked on the float64 oracle: the largest exponent is in the hundreds (exp() of it is
    not a float32), and a row's softplus argument is past the threshold of 20"""
    (img, pc, mask), ref, _ = desc_ref("K70_C16_norm3")
    d = ref["dists"]
    z_pos = DESC_HP["log_scale"] * (d.diagonal() - DESC_HP["pos_margin"]).clamp_min(0) ** 2
    z_neg = DESC_HP["log_scale"] * (DESC_HP["neg_margin"] - d[mask == 0]).clamp_min(0) ** 2
    assert float(z_pos.max()) > 100 and float(z_neg.max()) > 100
    assert float(torch.tensor(float(z_neg.max()), dtype=torch.float32).exp()) == float("inf")


# ------------------------------------------------------------------------------------------------------------------- overlap_loss
SATURATED_IN = [0.0, 1.0, 1e-30, 0.5, 1 - 1e-7, 1e-7]
SATURATED_OUT = [0.0, 1.0, 0.5, 1e-7, 1 - 1e-7]


def _bce(s_in, s_out):
    s_in, s_out = s_in.clone().requires_grad_(), s_out.clone().requires_grad_()
    label = torch.cat([torch.ones_like(s_in), torch.zeros_like(s_out)])
    loss = torch.nn.BCELoss()(torch.cat([s_in, s_out]), label)
    (UP * loss).backward()
    return dict(loss=loss.detach(), gin=s_in.grad, gout=s_out.grad)


def _run_overlap(s_in, s_out):
    from cofii2p_amd.loss import overlap_loss

    a, b = s_in.to(DEV).requires_grad_(), s_out.to(DEV).requires_grad_()
    loss = overlap_loss(DEV, a, b)
    (UP * loss).backward()
    return dict(loss=loss.detach(), gin=a.grad, gout=b.grad)


@pytest.mark.parametrize("n_in,n_out", [(1, 0), (0, 1), (31, 32), (32, 32), (33, 32), (700, 300)])
def test_overlap_loss_against_float64_bceloss(n_in, n_out):
    g = gen(7 * n_in + n_out)
    s_in, s_out = torch.sigmoid(2 * torch.randn(n_in, generator=g)), torch.sigmoid(2 * torch.randn(n_out, generator=g))
    ref, r32 = _bce(s_in.double(), s_out.double()), _bce(s_in, s_out)
    got = _run_overlap(s_in, s_out)
    for k in ("loss", "gin", "gout"):
        if ref[k].numel() == 0:   # the empty side has an empty gradient
            assert got[k] is None or got[k].numel() == 0
            continue
        assert got[k].shape == ref[k].shape
        e = err(got[k], ref[k])
        report("overlap_loss", "(%d, %d)" % (n_in, n_out), k, e, err(r32[k], ref[k]))
        assert e <= TOL, (k, e)


def test_overlap_loss_saturated_scores():
    """scores of exactly 0 and 1 (log clamped at -100, gradient denominator clamped at 1e-12) and next to them: the gradients reach
    9e10 and are compared entry by entry"""
    s_in, s_out = torch.tensor(SATURATED_IN, dtype=torch.float32), torch.tensor(SATURATED_OUT, dtype=torch.float32)
    ref, r32 = _bce(s_in.double(), s_out.double()), _bce(s_in, s_out)
    assert float(ref["gin"].abs().max()) > 1e10
    got = _run_overlap(s_in, s_out)
    e = err(got["loss"], ref["loss"])
    report("overlap_loss", "saturated", "loss", e, err(r32["loss"], ref["loss"]))
    assert e <= TOL
    for k in ("gin", "gout"):
        g, r = got[k].cpu().double(), ref[k]
        assert torch.isfinite(g).all()
        worst = float(((g - r).abs() / r.abs().clamp_min(1e-300)).max())
        worst32 = float(((r32[k].double() - r).abs() / r.abs().clamp_min(1e-300)).max())
        report("overlap_loss", "saturated", k + " (entry-wise)", worst, worst32)
        assert bool(((g - r).abs() <= TOL * r.abs()).all()), (k, g, r)


# --------------------------------------------------------------------------------------------------------------- fine_circle_loss
def _circle_inputs(case):
    """-> patches (K, C, 4, 4), pc (K, C), rel (K,), zero: None | ("patch", k, p) | ("pc", k)"""
    K, C, zero = {"K1_C1": (1, 1, None), "K5_C13": (5, 13, None), "K65_C64": (65, 64, None), "K200_C12": (200, 12, None),
                  "K5_C13_zero_positive_pixel": (5, 13, "pos"), "K6_C13_zero_negative_pixel": (6, 13, "neg"),
                  "K7_C13_zero_descriptor": (7, 13, "pc")}[case]
    g = gen(1000 * K + C)
    # norms far from 1: every pixel and every descriptor has a scale of its own
    patches = torch.randn(K, C, 4, 4, generator=g) * 10.0 ** (4 * torch.rand(K, 1, 4, 4, generator=g) - 2)
    pc = torch.randn(K, C, generator=g) * 10.0 ** (2 * torch.rand(K, 1, generator=g) - 1)
    rel = torch.randint(0, 16, (K,), generator=g)
    rel[-1] = 15
    if K > 1:
        rel[0] = 0
    where = None
    if zero == "pos":
        k, p = 2, int(rel[2])
        patches[k, :, p // 4, p % 4] = 0.0
        where = ("patch", k, p)
    elif zero == "neg":
        k, p = 3, (int(rel[3]) + 5) % 16
        patches[k, :, p // 4, p % 4] = 0.0
        where = ("patch", k, p)
    elif zero == "pc":
        pc[4, :] = 0.0
        where = ("pc", 4)
    return patches, pc, rel, where


CIRCLE_CASES = ["K1_C1", "K5_C13", "K65_C64", "K200_C12", "K5_C13_zero_positive_pixel", "K6_C13_zero_negative_pixel",
                "K7_C13_zero_descriptor"]


def _oracle_circle(patches, pc, rel):
    patches, pc = patches.clone().requires_grad_(), pc.clone().requires_grad_()
    loss = LO.fine_circle_loss(patches, pc, rel)
    (UP * loss).backward()
    return dict(loss=loss.detach(), gpatches=patches.grad, gpc=pc.grad)


@functools.lru_cache(maxsize=None)
def circle_ref(case):
    patches, pc, rel, where = _circle_inputs(case)
    r64, r32 = _oracle_circle(patches.double(), pc.double(), rel), _oracle_circle(patches, pc, rel)
    assert all(torch.isfinite(v).all() for v in list(r64.values()) + list(r32.values())), "the oracle itself must be finite on " + case
    return (patches, pc, rel, where), r64, r32


def _run_circle(patches, pc, rel):
    from cofii2p_amd.loss import fine_circle_loss

    a, b = patches.to(DEV).requires_grad_(), pc.to(DEV).requires_grad_()
    loss = fine_circle_loss(DEV, a, b, rel.to(DEV), num_kpt=patches.shape[0])
    (UP * loss).backward()
    return dict(loss=loss.detach(), gpatches=a.grad, gpc=b.grad)


def _circle_c1_allowance(patches, pc):
    """C = 1: cos(x, y) = sign(x y), so d cos / d x = y / (|x| |y|) - cos x / |x|^2 is the difference of two equal terms of size
    1 / |x| (1 / |y| for y).  |d L / d cos| <= UP / K * gamma * max(ap, an) <= UP / K * 5 * 2.2 (ap <= 1 + 1 + m, m = 0.2), and the
    descriptor's gradient sums 16 pixels.  A float32 evaluation leaves at most a few ulp of those terms: TOL times them is generous
    and still five orders of magnitude below a gradient that had lost one of the two terms."""
    K = patches.shape[0]
    bound = UP / K * 5.0 * 2.2
    return TOL * bound / patches.double().abs(), TOL * 16 * bound / pc.double().abs()


@pytest.mark.parametrize("case", CIRCLE_CASES)
def test_fine_circle_loss_against_float64_oracle(lib, case):
    """loss, d patches, d pc (non-unit upstream gradient) within TOL of the float64 oracle, the entries at a zero vector on their own;
    a second call gives the same bits"""
    (patches, pc, rel, where), ref, r32 = circle_ref(case)
    assert int(rel.max()) == 15 and (patches.shape[0] == 1 or int(rel.min()) == 0)
    got = _run_circle(patches, pc, rel)
    e = err(got["loss"], ref["loss"])
    report("fine_circle_loss", case, "loss", e, err(r32["loss"], ref["loss"]))
    assert e <= TOL, e
    again = _run_circle(patches, pc, rel)
    for k in got:
        assert torch.equal(got[k], again[k]), (case, k)
    if patches.shape[1] == 1:
        # a bound on |got| alone would pass a kernel that wrote nothing into zeroed memory: the same call through the C ABI on
        # sentinel-filled gradient buffers must overwrite every entry, with the bits the wrapper returned
        K = patches.shape[0]
        gpt, gpf = torch.full((K, 1, 16), SENTINEL, device=DEV), torch.full((K, 1), SENTINEL, device=DEV)
        rc, loss, _ = _abi_circle(lib, patches.reshape(K, 1, 16).to(DEV), pc.to(DEV), rel.to(DEV), gpt, gpf)
        assert rc == 0 and torch.equal(loss.reshape(()), got["loss"])
        assert torch.equal(gpt.reshape(patches.shape), got["gpatches"]) and torch.equal(gpf, got["gpc"])
        for k, allow in zip(("gpatches", "gpc"), _circle_c1_allowance(patches, pc)):
            assert float(allow.max()) < 1.0 < abs(SENTINEL)
            assert bool((ref[k].abs() <= allow).all()), "the reference's gradient is zero up to cancellation"
            assert bool((got[k].cpu().double().abs() <= allow).all()), (k, got[k])
        return
    # the entries at a zero vector are 1e5 ... 1e8 (1 / eps of the cosine): on their own, and kept out of the rest
    sel = {k: torch.zeros_like(ref[k], dtype=torch.bool) for k in ("gpatches", "gpc")}
    if where is not None and where[0] == "patch":
        sel["gpatches"][where[1], :, where[2] // 4, where[2] % 4] = True
    elif where is not None:
        sel["gpc"][where[1], :] = True
    for k in ("gpatches", "gpc"):
        g = got[k].cpu()
        assert g.shape == ref[k].shape
        if sel[k].any():
            assert 1e4 < float(ref[k][sel[k]].abs().max()) < 1e9
            e = err(g[sel[k]], ref[k][sel[k]])
            report("fine_circle_loss", case, k + " at the zero vector", e, err(r32[k][sel[k]], ref[k][sel[k]]))
            assert e <= TOL, (k, e)
        e = err(g[~sel[k]], ref[k][~sel[k]])
        report("fine_circle_loss", case, k, e, err(r32[k][~sel[k]], ref[k][~sel[k]]))
        assert e <= TOL, (k, e)


# ------------------------------------------------------------------------------------------------------------------- the C ABI
def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def lib():
    from cofii2p_amd import _lib

    assert torch.cuda.is_available()
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _abi_desc(lib, img, pc, mask, gimg=None, gpc=None, upstream=True, ws_short=0, ld=None):
    """cofi_desc_loss on 2-D views of any row stride -> (rc, loss, dists)"""
    C, K = img.shape
    loss, dists = torch.zeros(1, device=DEV), torch.zeros(K, K, device=DEV)
    g = torch.full((1,), UP, device=DEV) if upstream else None
    nbytes = lib.cofi_desc_loss_workspace(K)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    ld = ld or {}
    rc = lib.cofi_desc_loss(P(img), ld.get("i", img.stride(0)), P(pc), ld.get("p", pc.stride(0)), P(mask), C, K, DESC_HP["pos_margin"],
                            DESC_HP["neg_margin"], DESC_HP["log_scale"], P(loss), P(dists), P(g),
                            P(gimg), ld.get("gi", gimg.stride(0) if gimg is not None else 0),
                            P(gpc), ld.get("gp", gpc.stride(0) if gpc is not None else 0), P(ws), nbytes - ws_short, _stream())
    return rc, loss, dists


SENTINEL = -12345.5


def test_desc_loss_abi_row_strides_wider_than_K(lib):
    """img, pc, grad_img, grad_pc as column slices of wider buffers (ldi, ldp, ldgi, ldgp > K, all different): the same bits as the
    contiguous call, and not one padding column of the gradient buffers is written"""
    C, K = 12, 70
    g = gen(5)
    img, pc, mask = _unit_cols(C, K, g).to(DEV), _unit_cols(C, K, g).to(DEV), torch.eye(K, device=DEV)
    gi0, gp0 = torch.zeros(C, K, device=DEV), torch.zeros(C, K, device=DEV)
    rc, loss0, dists0 = _abi_desc(lib, img, pc, mask, gi0, gp0)
    assert rc == 0
    wi, wp = torch.randn(C, K + 9, generator=g).to(DEV), torch.randn(C, K + 5, generator=g).to(DEV)
    wi[:, 4:4 + K], wp[:, 2:2 + K] = img, pc
    wgi, wgp = torch.full((C, K + 7), SENTINEL, device=DEV), torch.full((C, K + 3), SENTINEL, device=DEV)
    rc, loss1, dists1 = _abi_desc(lib, wi[:, 4:4 + K], wp[:, 2:2 + K], mask, wgi[:, 6:6 + K], wgp[:, 1:1 + K])
    assert rc == 0
    assert wi.stride(0) > K and wp.stride(0) > K and wgi.stride(0) > K and wgp.stride(0) > K
    assert torch.equal(loss0, loss1) and torch.equal(dists0, dists1)
    assert torch.equal(wgi[:, 6:6 + K], gi0) and torch.equal(wgp[:, 1:1 + K], gp0)
    assert float(gi0.abs().sum()) > 0 and float(gp0.abs().sum()) > 0
    for buf, lo in ((wgi, 6), (wgp, 1)):
        assert bool((buf[:, :lo] == SENTINEL).all()) and bool((buf[:, lo + K:] == SENTINEL).all())
    # one gradient only
    only = torch.full((C, K + 7), SENTINEL, device=DEV)
    rc, _, _ = _abi_desc(lib, wi[:, 4:4 + K], wp[:, 2:2 + K], mask, None, only[:, 6:6 + K])
    assert rc == 0 and torch.equal(only[:, 6:6 + K], gp0) and bool((only[:, :6] == SENTINEL).all()) and bool((only[:, 6 + K:] == SENTINEL).all())


def _abi_circle(lib, patches, pc, rel, gpatches=None, gpc=None, upstream=True, ld=None):
    K, C = pc.shape
    loss, per = torch.zeros(1, device=DEV), torch.zeros(K, device=DEV)
    g = torch.full((1,), UP, device=DEV) if upstream else None
    ld = ld or {}
    rc = lib.cofi_fine_circle_loss(P(patches), P(pc), ld.get("p", pc.stride(0)), P(rel), K, C, 0.2, 5.0, P(loss), P(per), P(g), P(gpatches),
                                   P(gpc), ld.get("g", gpc.stride(0) if gpc is not None else 0), _stream())
    return rc, loss, per


def test_fine_circle_loss_abi_row_strides_wider_than_C(lib):
    K, C = 9, 13
    g = gen(6)
    patches, pc = torch.randn(K, C, 16, generator=g).to(DEV), torch.randn(K, C, generator=g).to(DEV)
    rel = torch.randint(0, 16, (K,), generator=g).to(DEV)
    gpt0, gpc0 = torch.zeros(K, C, 16, device=DEV), torch.zeros(K, C, device=DEV)
    rc, loss0, per0 = _abi_circle(lib, patches, pc, rel, gpt0, gpc0)
    assert rc == 0
    wp = torch.randn(K, C + 6, generator=g).to(DEV)
    wp[:, 3:3 + C] = pc
    gpt1, wg = torch.zeros(K, C, 16, device=DEV), torch.full((K, C + 4), SENTINEL, device=DEV)
    rc, loss1, per1 = _abi_circle(lib, patches, wp[:, 3:3 + C], rel, gpt1, wg[:, 2:2 + C])
    assert rc == 0
    assert torch.equal(loss0, loss1) and torch.equal(per0, per1) and torch.equal(gpt0, gpt1) and torch.equal(wg[:, 2:2 + C], gpc0)
    assert float(gpc0.abs().sum()) > 0 and float(gpt0.abs().sum()) > 0
    assert bool((wg[:, :2] == SENTINEL).all()) and bool((wg[:, 2 + C:] == SENTINEL).all())


def test_loss_abi_argument_checks(lib):
    """every refusal returns before a launch"""
    C, K = 4, 6
    z = lambda *s: torch.zeros(*s, device=DEV)
    img, pc, mask, gi, gp = z(C, K), z(C, K), z(K, K), z(C, K), z(C, K)
    assert _abi_desc(lib, img, pc, mask, gi, gp)[0] == 0
    for which in ("i", "p", "gi", "gp"):
        assert _abi_desc(lib, img, pc, mask, gi, gp, ld={which: K - 1})[0] == COFI_EINVAL, which
    assert _abi_desc(lib, img, pc, mask, gi, None, upstream=False)[0] == COFI_EINVAL
    assert _abi_desc(lib, img, pc, mask, None, gp, upstream=False)[0] == COFI_EINVAL
    assert _abi_desc(lib, img, pc, mask, gi, gp, ws_short=1)[0] == COFI_EWORKSPACE
    assert lib.cofi_desc_loss_workspace(K) == 4 * (4 * K + K * K)
    patches, fpc, rel = z(K, C, 16), z(K, C), torch.zeros(K, dtype=torch.int64, device=DEV)
    gpt, gpc = z(K, C, 16), z(K, C)
    assert _abi_circle(lib, patches, fpc, rel, gpt, gpc)[0] == 0
    assert _abi_circle(lib, patches, fpc, rel, gpt, gpc, ld={"p": C - 1})[0] == COFI_EINVAL
    assert _abi_circle(lib, patches, fpc, rel, gpt, gpc, ld={"g": C - 1})[0] == COFI_EINVAL
    assert _abi_circle(lib, patches, fpc, rel, gpt, None, upstream=False)[0] == COFI_EINVAL
    assert _abi_circle(lib, patches, fpc, rel, None, gpc, upstream=False)[0] == COFI_EINVAL
    s, loss, g = torch.full((3,), 0.5, device=DEV), z(1), torch.ones(1, device=DEV)
    assert lib.cofi_overlap_loss(P(s), 3, P(s), 3, P(loss), None, None, None, _stream()) == 0
    assert lib.cofi_overlap_loss(P(s), 0, P(s), 0, P(loss), P(g), P(s), P(s), _stream()) == COFI_EINVAL   # n_in + n_out == 0
    assert lib.cofi_overlap_loss(P(s), 3, P(s), 3, None, None, None, None, _stream()) == COFI_EINVAL     # nothing asked for
    assert lib.cofi_overlap_loss(P(s), -1, P(s), 3, P(loss), None, None, None, _stream()) == COFI_EINVAL
    # a side needs a pointer exactly when it is not empty (torch's empty tensors have a NULL data pointer)
    assert lib.cofi_overlap_loss(None, 3, P(s), 3, P(loss), None, None, None, _stream()) == COFI_EINVAL
    assert lib.cofi_overlap_loss(P(s), 3, None, 3, P(loss), None, None, None, _stream()) == COFI_EINVAL
    assert lib.cofi_overlap_loss(None, 1, None, 0, P(loss), None, None, None, _stream()) == COFI_EINVAL
    assert lib.cofi_overlap_loss(None, 0, None, 1, P(loss), None, None, None, _stream()) == COFI_EINVAL
    with_ptr, without = z(1), z(1)
    for a, b in (((P(s), 3, P(s), 0), (P(s), 3, None, 0)), ((P(s), 0, P(s), 3), (None, 0, P(s), 3))):
        assert lib.cofi_overlap_loss(*a, P(with_ptr), None, None, None, _stream()) == 0
        assert lib.cofi_overlap_loss(*b, P(without), None, None, None, _stream()) == 0
        assert torch.equal(with_ptr, without) and abs(float(without) - 0.6931472) < 1e-6   # -log(0.5), whichever side
    torch.cuda.synchronize()
