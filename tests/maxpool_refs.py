"""Plain reference of the neighbour max-pool (model/kpconv/functional.py:53-66), per frame:
    out[m, c] = max_h x[idx[m, h], c]     with a zero row behind every index outside [0, N)
as the kernels define it (cofi_neighbor_maxpool, cofi_neighbor_maxpool_slice): `frames` equally sized frames stacked along the rows of x
and idx, indices frame-local.  A NaN entry is skipped (fmaxf), a row whose entries are all NaN gives -inf."""
import numpy as np
import torch


def neighbor_maxpool_ref(x, idx, frames: int = 1):
    """x (frames * N, C) float32, idx (frames * M, H) integer -> (frames * M, C) float32 (numpy)"""
    x = np.asarray(x, dtype=np.float32)
    idx = np.asarray(idx).astype(np.int64)
    N, C = x.shape[0] // frames, x.shape[1]
    M, H = idx.shape[0] // frames, idx.shape[1]
    out = np.empty((frames * M, C), dtype=np.float32)
    for f in range(frames):
        xf = np.concatenate([x[f * N:(f + 1) * N], np.zeros((1, C), dtype=np.float32)])   # the zero row at N
        i = idx[f * M:(f + 1) * M]
        i = np.where((i >= 0) & (i < N), i, N)
        g = xf[i]                                                                        # (M, H, C)
        with np.errstate(invalid="ignore"):
            out[f * M:(f + 1) * M] = np.fmax.reduce(g, axis=1, initial=-np.inf)             # fmax skips NaN, as fmaxf does
    return out


def neighbor_maxpool_ref_torch(x: torch.Tensor, idx: torch.Tensor, frames: int = 1) -> torch.Tensor:
    return torch.from_numpy(neighbor_maxpool_ref(x.detach().cpu().numpy(), idx.detach().cpu().numpy(), frames))
