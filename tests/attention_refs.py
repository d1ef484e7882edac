"""Plain-torch restatements for the softmax attention kernels (csrc/attention.hip, attention_x6.inc, attention_parts.h) and the fused LoFTR
layer tail (csrc/transformer_tail.hip), with a dtype argument: float64 is the yardstick of the kernel tests, float32 the level a plain
evaluation reaches.  Matrices throughout: q (L, H*32), k / v (S, H*32), heads side by side in the columns; stack mode: frame f owns rows
f*L .. (f+1)*L of q and f*S .. (f+1)*S of k / v, and q_colscale is (frames, H*32).

THE BOUND (error_bound).  With u = 2^-24, D = 32, t_s = log2(e) / sqrt(D) * sum_d q_d k_d the base-2 score of key s, m = max_s t_s and
p_s = 2^(t_s - m) / sum_s' 2^(t_s' - m):

    delta[l, h] = C1 * u * max_s( log2(e) / sqrt(D) * sum_d |q_d k_d|  +  |t_s|  +  |m| )
    bound[l, v] = (2 * ln(2) * delta  +  C2 * (S + 2 D) * u) * sum_s p_s |v_s|

Derivation, first order in u, for any summation order.
  * The exponent t_s - m of a weight.  The scaled query (q * colscale) * (log2(e) / sqrt(D)) rounds twice (2 u per product); each of the
    D products and D - 1 additions of the dot product rounds once and a term passes through at most D of them (D u); the three products
    that the six-product split drops (mid.lo, lo.mid, lo.lo) are each below u of the product (3 u): (D + 5) u on sum_d |q_d k_d| in the
    worst case.  The subtraction of the running maximum rounds once, u (|t_s| + |m|), and every later change of the maximum (online
    rescale, merge of the waves, merge of the slots) subtracts two maxima again - at most 4 u on |t_s| + |m|.  One constant C1 for all
    three terms: an exponent is off by at most delta, a normalised weight by the factor 2^(2 delta) (its own exponent and the
    normaliser's), i.e. by 2 ln(2) delta relative.
  * Everything that is relative to p_s |v_s|: the hardware exp2 (1 ulp = 2 u, in the numerator and in the row sum), the S products and
    additions of sum_s p_s v_s and the S additions of the row sum (a term passes through at most S of each), the multiplications by the
    rescale factors, the three dropped products of the second contraction, the reciprocal and the final product: a multiple of
    (S + 2 D) u - the 2 D holds what does not grow with S.
  * The worst case (C1 = D + 5 = 37, C2 = 3) is never met: rounding errors of a sum of n terms add up like sqrt(n), not like n, and a
    bound that loose passes a kernel that reads K from its bf16 hi plane alone.  So the constants are the smallest of this form for which a
    plain float32 evaluation stays under HALF the bound and the emulated six-product split arithmetic under the bound, over every case
    and regime below (tests/test_attention_refs_cpu.py prints the table): the factor 2 is the room for the kernels' other summation order.

    C1 = 2, C2 = 1/8   (powers of two: with C1 = 1 the peaked and sentinel regimes need C2 = 1/2, four times the bound on flat inputs,
    where the second term is all there is; with C1 = 2, C2 = 1/16 misses the float32 condition at S = 5).

  Measured with them (largest error / bound over CASES x REGIMES, tests/test_attention_refs_cpu.py): float32 restatement 0.38 (limit 0.5),
  emulated six-product split 0.28 (limit 1.0); the smallest mutation - K rounded to its bf16 hi plane, S = 923 - is 4.6 times the bound.
"""
import functools
import math

import torch
import torch.nn.functional as F

D = 32
U = 2.0 ** -24
LOG2E = 1.4426950408889634
C1, C2 = 2.0, 1.0 / 8


# ------------------------------------------------------------------------------------------------ the operator
def full_attention(q, k, v, q_colscale=None, nhead=4, dtype=torch.float64):
    """softmax(q k^T / sqrt(32)) v per head (oracle/cofi_oracle.py:full_attention, same operation order) on matrices."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    if q_colscale is not None:
        q = q * q_colscale.to(dtype)
    L, HD = q.shape
    S = k.shape[0]
    d = HD // nhead
    scores = torch.einsum("lhd,shd->hls", q.view(L, nhead, d), k.view(S, nhead, d)) / math.sqrt(d)
    return torch.einsum("hls,shd->lhd", scores.softmax(-1), v.view(S, nhead, d)).reshape(L, HD)


def bound_terms(q, k, v, q_colscale=None, nhead=4):
    """(E1, E2), float64, per element: bound = C1 * E1 + C2 * E2 (module docstring)."""
    q, k, v = q.double(), k.double(), v.double()
    if q_colscale is not None:
        q = q * q_colscale.double()
    L, HD = q.shape
    S = k.shape[0]
    d = HD // nhead
    c = LOG2E / math.sqrt(d)
    Q, K, V = q.view(L, nhead, d), k.view(S, nhead, d), v.view(S, nhead, d)
    t = c * torch.einsum("lhd,shd->hls", Q, K)
    a = c * torch.einsum("lhd,shd->hls", Q.abs(), K.abs())
    m = t.max(-1, keepdim=True).values
    delta = U * (a + t.abs() + m.abs()).max(-1).values                   # (H, L), without C1
    pv = torch.einsum("hls,shd->lhd", torch.softmax(t * math.log(2.0), -1), V.abs())
    e1 = (2 * math.log(2.0) * delta.t()[:, :, None] * pv).reshape(L, HD)
    e2 = ((S + 2 * d) * U * pv).reshape(L, HD)
    return e1, e2


def error_bound(q, k, v, q_colscale=None, nhead=4):
    """Per element, float64: the bound on |out32 - out64| of the module docstring."""
    e1, e2 = bound_terms(q, k, v, q_colscale, nhead)
    return C1 * e1 + C2 * e2


def planes3(x):
    """fp32 -> (hi, mid, lo) as fp32 tensors holding bf16 values: bf16(x) (RNE), bf16 of the residual, bf16 of its residual."""
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    return hi, mid, (r - mid).bfloat16().float()


def _six(eq, a, b):
    """the six plane products that attention_x6.inc names, small terms first, accumulated in fp32: (A plane, B plane) =
    (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi)"""
    acc = None
    for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)):
        term = torch.einsum(eq, a[i], b[j])
        acc = term if acc is None else acc + term
    return acc


def split6_attention(q, k, v, q_colscale=None, nhead=4):
    """The operator in float32 torch with q * scale, k, v and p cut into three bf16 planes each and every contraction the six plane
    products of attention_x6.inc: the ARITHMETIC of the split kernel (base-2 scores, weights relative to the row maximum, one division
    at the end) on the CPU - not its tiling, its summation order or its online rescale."""
    q, k, v = q.float(), k.float(), v.float()
    if q_colscale is not None:
        q = q * q_colscale.float()
    L, HD = q.shape
    S = k.shape[0]
    d = HD // nhead
    qs = q * torch.tensor(LOG2E / math.sqrt(d), dtype=torch.float32)
    Q = [p.view(L, nhead, d) for p in planes3(qs)]
    K = [p.view(S, nhead, d) for p in planes3(k)]
    V = [p.view(S, nhead, d) for p in planes3(v)]
    t = _six("shd,lhd->hls", K, Q)
    p = torch.exp2(t - t.max(-1, keepdim=True).values)
    o = _six("shd,hls->lhd", V, planes3(p))
    return (o / p.sum(-1).t()[:, :, None]).reshape(L, HD)


# ------------------------------------------------------------------------------------------------ the key split
QG, KPH, MAX_KS = 2, 4, 8   # COFI_ATTN_QG, COFI_ATTN_KPH, COFI_ATTN_MAX_KS (csrc/attention_parts.h)


def _cdiv(a, b):
    return -(-a // b)


def key_layout(L, S, H, frames, ncu=256):
    """attn_layout (csrc/attention_parts.h) restated: which split of the key blocks a call of this shape runs on a device of `ncu`
    compute units.  ranges: (first key block, blocks) of every key range, as the kernels compute them."""
    P, QB = _cdiv(S, 32), _cdiv(L, 32)
    QSB = _cdiv(QB, QG)
    sp = frames * H * QSB
    light = int(sp * 2 >= ncu)
    n = ncu * (2 if light else 1)
    best, best_cost = 1, 1e30
    for ks in range(1, min(MAX_KS, P) + 1):
        cost = _cdiv(sp * ks, n) * (_cdiv(_cdiv(P, ks), KPH) + 1.5)
        if cost < best_cost - 1e-9:
            best, best_cost = ks, cost
    base, rem = divmod(P, best)
    ranges = [(ks * base + min(ks, rem), base + (1 if ks < rem else 0)) for ks in range(best)]
    return {"P": P, "QB": QB, "QSB": QSB, "KS": best, "light": light, "nwg": sp * best, "ranges": ranges}


# ------------------------------------------------------------------------------------------------ the layer tail
def layer_tail(msg, x, w, dtype=torch.float64, eps=1e-5):
    """What cofi_loftr_tail computes from the attention output `msg` and the layer input `x` (transformer.py:57-64), `w`: reference-named
    weights.  -> dict: out = x + LN2(relu([x | LN1(msg Wm^T)] W0^T) W2^T); q / k / v = out W^T for the projection weights present;
    l2 = F.normalize(out, dim=1); part = the {sum, sum of squares} of the columns of [q | k | v] over every 32-row slab (the last one
    may be partial), (slabs, 3 C, 2)."""
    w = {n: t.to(dtype) for n, t in w.items()}
    msg, x = msg.to(dtype), x.to(dtype)
    C = x.shape[1]
    m = F.layer_norm(msg @ w["merge.weight"].t(), (C,), w["norm1.weight"], w["norm1.bias"], eps)
    h = torch.relu(torch.cat([x, m], 1) @ w["mlp.0.weight"].t()) @ w["mlp.2.weight"].t()
    out = x + F.layer_norm(h, (C,), w["norm2.weight"], w["norm2.bias"], eps)
    res = {"out": out, "l2": F.normalize(out, dim=1)}
    for n in "qkv":
        if n + "_proj.weight" in w:
            res[n] = out @ w[n + "_proj.weight"].t()
    if all(n in res for n in "qkv"):
        res["part"] = column_partials(torch.cat([res["q"], res["k"], res["v"]], 1))
    return res


def column_partials(y, slab=32):
    """(rows, N) -> (ceil(rows / slab), N, 2): {sum, sum of squares} of every column over every slab of rows"""
    return torch.stack([torch.stack([b.sum(0), (b * b).sum(0)], -1) for b in y.split(slab)])


def tail_weights(seed=21):
    """the weights of test_loftr_tail_fused_successors (tests/test_ops_gpu.py), reference-named, float32"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"q_proj.weight": rn(128, 128) / 11, "k_proj.weight": rn(128, 128) / 11, "v_proj.weight": rn(128, 128) / 11, "merge.weight": rn(128, 128) / 11,
            "mlp.0.weight": rn(256, 256) / 16, "mlp.2.weight": rn(128, 256) / 16, "norm1.weight": 1 + 0.1 * rn(128), "norm1.bias": 0.1 * rn(128),
            "norm2.weight": 1 + 0.1 * rn(128), "norm2.bias": 0.1 * rn(128)}


# ------------------------------------------------------------------------------------------------ cases, regimes, mutations
# (frames, L, S, nhead)
EDGE_CASES = [(1, 1, 1, 4), (1, 1, 33, 4), (1, 31, 32, 4), (1, 32, 31, 4), (1, 33, 33, 4), (1, 65, 129, 4), (1, 96, 5, 4)]
FRAME_CASES = [(3, 40, 50, 4), (2, 33, 257, 4)]
LIGHT_CASES = [(16, 128, 70, 4)]   # frames * H * QSB = 128 workgroups per key range: the smallest that is "light" on 256 compute units
HEAD_CASES = [(1, 70, 100, 1), (1, 70, 100, 2), (1, 70, 100, 8)]
# one case per KS = 1 .. 8 on 256 compute units: L = 64, H = 4, one frame -> 4 workgroups per key range, the split depends on P alone
# and is the smallest ks with ceil(ceil(P / ks) / 4) == 1.  S = 32 (4 n + 1) - 5 gives P = 4 n + 1 -> KS = n + 1; P = 9 splits evenly
# (3 x 3), so KS = 3 takes P = 10 (4 + 3 + 3).  KS = 1 has one range by definition.
KS_CASES = {1: (1, 64, 27, 4), 2: (1, 64, 155, 4), 3: (1, 64, 315, 4), 4: (1, 64, 411, 4), 5: (1, 64, 539, 4), 6: (1, 64, 667, 4),
            7: (1, 64, 795, 4), 8: (1, 64, 923, 4)}
CASES = EDGE_CASES + FRAME_CASES + LIGHT_CASES + HEAD_CASES + list(KS_CASES.values())
# KS every case was chosen for, on 256 compute units (tests assert it through key_layout)
EXPECTED_KS = {(1, 1, 1, 4): 1, (1, 1, 33, 4): 1, (1, 31, 32, 4): 1, (1, 32, 31, 4): 1, (1, 33, 33, 4): 1, (1, 65, 129, 4): 2, (1, 96, 5, 4): 1,
               (3, 40, 50, 4): 1, (2, 33, 257, 4): 3, (16, 128, 70, 4): 1, (1, 70, 100, 1): 1, (1, 70, 100, 2): 1, (1, 70, 100, 8): 1}
EXPECTED_KS.update({c: ks for ks, c in KS_CASES.items()})

REGIMES = ["flat", "peaked", "sentinel_up", "sentinel_down", "v_1e4", "v_1e-4"]


def case_id(case):
    return "f%d-L%d-S%d-H%d" % case


def col_scale(q, eps=1e-12):
    """The token-axis F.normalize of the queries (transformer.py:53) as a per-column scale."""
    return 1 / torch.clamp(q.norm(dim=0), min=eps)


def sentinel_positions(S):
    """frame-local keys that get a planted key: the first and the last key of every 32-block - every key range starts and ends on one,
    whatever the split - and S - 1"""
    pos = set()
    for kb in range(_cdiv(S, 32)):
        pos.update((kb * 32, min(kb * 32 + 31, S - 1)))
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def case_inputs(case, regime):
    """-> dict q (frames*L, HD), k / v (frames*S, HD), cs (frames, HD) or None; float32, deterministic.
    flat: q_colscale = 1 / ||q[:, c]|| per frame, as the product runs it - every key weighs about 1 / S.
    peaked: keys times 8, no scale.
    sentinel_up / sentinel_down: peaked, plus keys c * q[l] planted at sentinel_positions in ascending / descending strength - the online
    rescale runs with the maximum arriving last / first.
    v_1e4 / v_1e-4: flat with v times 1e4 / 1e-4."""
    frames, L, S, H = case
    HD = H * D
    g = torch.Generator().manual_seed(100000 * frames + 1000 * L + 10 * S + H)
    q = 0.5 * torch.randn(frames * L, HD, generator=g)
    k = torch.randn(frames * S, HD, generator=g)
    v = torch.randn(frames * S, HD, generator=g)
    cs = None
    if regime in ("flat", "v_1e4", "v_1e-4"):
        cs = torch.stack([col_scale(q[f * L:(f + 1) * L]) for f in range(frames)])
        if regime != "flat":
            v = v * float(regime[2:])
    elif regime in ("peaked", "sentinel_up", "sentinel_down"):
        k = 8.0 * k
        if regime != "peaked":
            pos = sentinel_positions(S)
            n = len(pos)
            for f in range(frames):
                for i, s in enumerate(pos):
                    j = i if regime == "sentinel_up" else n - 1 - i
                    strength = 8.0 + 16.0 * j / max(n - 1, 1)
                    k[f * S + s] = strength * q[f * L + (7 * i) % L]
    else:
        raise ValueError(regime)
    return {"q": q, "k": k, "v": v, "cs": cs}


def frame_slices(case, inp, f):
    frames, L, S, H = case
    return (inp["q"][f * L:(f + 1) * L], inp["k"][f * S:(f + 1) * S], inp["v"][f * S:(f + 1) * S], None if inp["cs"] is None else inp["cs"][f])


def _per_frame(case, inp, fn):
    return torch.cat([fn(*frame_slices(case, inp, f)) for f in range(case[0])])


def reference(case, inp, dtype=torch.float64):
    """every frame against its own keys"""
    return _per_frame(case, inp, lambda q, k, v, cs: full_attention(q, k, v, cs, nhead=case[3], dtype=dtype))


def split6(case, inp):
    return _per_frame(case, inp, lambda q, k, v, cs: split6_attention(q, k, v, cs, nhead=case[3]))


def bound(case, inp):
    return _per_frame(case, inp, lambda q, k, v, cs: error_bound(q, k, v, cs, nhead=case[3]))


@functools.lru_cache(maxsize=None)
def reference_and_bound(case, regime):
    """(out64, bound) of case_inputs(case, regime): computed once, shared by the tests, never modified"""
    inp = case_inputs(case, regime)
    return reference(case, inp), bound(case, inp)


MUTATIONS = ["drop_last_key", "extra_key", "drop_block", "double_block", "frame_leak", "k_bf16_hi"]


def mutation_applicable(case, kind):
    frames, L, S, H = case
    if kind == "drop_last_key":
        return S > 1
    if kind in ("drop_block", "double_block"):
        return S > 32
    if kind == "frame_leak":
        return frames > 1
    if kind == "k_bf16_hi":
        return S > 1      # a single key weighs 1 whatever its score
    return True


def mutated(case, inp, kind):
    """The float64 restatement with one defect: a dropped key S - 1; one extra key row past S (the next frame's first row, or ones);
    one whole 32-key block dropped (the middle one); one block counted twice; frame f sees frame f + 1's keys (the last frame the
    first one's); k rounded to its bf16 hi plane."""
    frames, L, S, H = case
    assert mutation_applicable(case, kind)
    out = []
    for f in range(frames):
        q, k, v, cs = frame_slices(case, inp, f)
        if kind == "drop_last_key":
            k, v = k[:-1], v[:-1]
        elif kind == "extra_key":
            if f + 1 < frames:
                k, v = inp["k"][f * S:(f + 1) * S + 1], inp["v"][f * S:(f + 1) * S + 1]
            else:
                k, v = torch.cat([k, torch.ones(1, H * D)]), torch.cat([v, torch.ones(1, H * D)])
        elif kind in ("drop_block", "double_block"):
            kb = _cdiv(S, 32) // 2
            blk = slice(kb * 32, min(kb * 32 + 32, S))
            if kind == "drop_block":
                keep = [s for s in range(S) if not blk.start <= s < blk.stop]
                k, v = k[keep], v[keep]
            else:
                k, v = torch.cat([k, k[blk]]), torch.cat([v, v[blk]])
        elif kind == "frame_leak":
            _, k, v, _ = frame_slices(case, inp, (f + 1) % frames)
        elif kind == "k_bf16_hi":
            k = k.bfloat16().float()
        else:
            raise ValueError(kind)
        out.append(full_attention(q, k, v, cs, nhead=H))
    return torch.cat(out)
