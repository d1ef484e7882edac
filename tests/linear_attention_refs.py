"""Plain-torch restatement of LoFTR linear attention with a dtype argument: float64 is the yardstick of the kernel tests,
float32 the level a plain evaluation reaches.  Matrices throughout: q (L, H*D), k / v (S, H*D), heads side by side in the columns."""
import torch
import torch.nn.functional as F


def phi(x):
    """elu(x) + 1 = x + 1 for x > 0, exp(x) otherwise."""
    return torch.where(x > 0, x + 1, torch.exp(torch.clamp(x, max=0)))


def col_scale(q, eps=1e-12):
    """The token-axis F.normalize of the queries (dim = tokens) as a per-column scale."""
    return 1 / torch.clamp(q.norm(dim=0), min=eps)


def linear_attention(q, k, v, q_colscale=None, nhead=4, eps=1e-6, dtype=torch.float64):
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    L, HD = q.shape
    S = k.shape[0]
    D = HD // nhead
    if q_colscale is not None:
        q = q * q_colscale.to(dtype)
    Q, K = phi(q).view(L, nhead, D), phi(k).view(S, nhead, D)
    Vs = (v / S).view(S, nhead, D)
    KV = torch.einsum("shd,shv->hdv", K, Vs)
    Z = 1 / (torch.einsum("lhd,hd->lh", Q, K.sum(0)) + eps)
    return (torch.einsum("lhd,hdv->lhv", Q, KV) * Z[:, :, None] * S).reshape(L, HD)


def error_bound(q, k, v, q_colscale=None, nhead=4, eps=1e-6):
    """Per element 2 * (S + 2 D + 16) * 2^-24 * A[l, v], A = (sum_d phi(q)[l, d] * sum_s phi(k)[s, d] |v[s, v]|) * Z[l], in float64: a
    bound on |out32 - out64| for any summation order (each of the S + D products and sums rounds once, the normaliser as many times
    again; 16 covers exp, the scale and the divisions)."""
    q, k, v = q.double(), k.double(), v.double()
    L, HD = q.shape
    S = k.shape[0]
    D = HD // nhead
    if q_colscale is not None:
        q = q * q_colscale.double()
    Q, K = phi(q).view(L, nhead, D), phi(k).view(S, nhead, D)
    KA = torch.einsum("shd,shv->hdv", K, v.abs().view(S, nhead, D))
    Z = 1 / (torch.einsum("lhd,hd->lh", Q, K.sum(0)) + eps)
    A = (torch.einsum("lhd,hdv->lhv", Q, KA) * Z[:, :, None]).reshape(L, HD)
    return 2 * (S + 2 * D + 16) * 2.0 ** -24 * A


def loftr_layer(w, x, src, nhead=4, dtype=torch.float64, attention="linear"):
    """One LoFTR encoder layer (projections, token-axis query normalisation, attention, merge, LayerNorm, MLP, LayerNorm, residual) on
    (L, C) / (S, C) matrices; `w`: reference-named weights.  attention='linear' only (the softmax layer has its own oracle)."""
    assert attention == "linear"
    w = {n: t.to(dtype) for n, t in w.items()}
    x, src = x.to(dtype), src.to(dtype)
    C = x.shape[1]
    q = F.normalize(x @ w["q_proj.weight"].t(), dim=0)
    k, v = src @ w["k_proj.weight"].t(), src @ w["v_proj.weight"].t()
    msg = linear_attention(q, k, v, nhead=nhead, dtype=dtype)
    msg = F.layer_norm(msg @ w["merge.weight"].t(), (C,), w["norm1.weight"], w["norm1.bias"])
    h = torch.relu(torch.cat([x, msg], 1) @ w["mlp.0.weight"].t()) @ w["mlp.2.weight"].t()
    return x + F.layer_norm(h, (C,), w["norm2.weight"], w["norm2.bias"])


CASES = [(48, 80), (1, 1), (33, 1), (7, 65), (64, 63), (64, 64), (130, 1280)]   # (L, S); keys scaled by 8


def case_inputs(L, S, nhead=4, D=32, seed=0):
    g = torch.Generator().manual_seed(1000 * L + S + seed)
    q = 0.5 * torch.randn(L, nhead * D, generator=g)
    k = 8.0 * torch.randn(S, nhead * D, generator=g)
    v = torch.randn(S, nhead * D, generator=g)
    return q, k, v
