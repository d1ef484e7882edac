"""tests/maxpool_refs.py (the reference of the GPU max-pool tests) against the CPU oracle's neighbor_maxpool on tiny inputs."""
import numpy as np
import pytest
import torch

import cofi_oracle as O
import maxpool_refs as R


@pytest.mark.parametrize("N,M,H,C", [(1, 1, 1, 1), (7, 9, 5, 3), (12, 4, 16, 8), (30, 30, 7, 5)])
def test_reference_matches_oracle(N, M, H, C):
    g = np.random.default_rng(N * 100 + H)
    x = g.standard_normal((N, C)).astype(np.float32)
    idx = g.integers(0, N + 1, (M, H))           # N = the shadow index: the oracle's pad row
    idx[0] = N                                   # a row of shadows only -> zeros
    ref = R.neighbor_maxpool_ref(x, idx)
    assert ref.dtype == np.float32 and ref.shape == (M, C)
    assert torch.equal(torch.from_numpy(ref), O.neighbor_maxpool(torch.from_numpy(x), torch.from_numpy(idx)))
    assert not ref[0].any()


def test_reference_frames_are_independent():
    g = np.random.default_rng(3)
    N, M, H, C, F = 6, 5, 4, 3, 3
    x = g.standard_normal((F * N, C)).astype(np.float32)
    idx = g.integers(0, N + 1, (F * M, H))
    ref = R.neighbor_maxpool_ref(x, idx, frames=F)
    for f in range(F):
        one = O.neighbor_maxpool(torch.from_numpy(x[f * N:(f + 1) * N]), torch.from_numpy(idx[f * M:(f + 1) * M]))
        assert torch.equal(torch.from_numpy(ref[f * M:(f + 1) * M]), one)


def test_reference_range_rule_and_nan():
    x = np.array([[-1.0, 2.0], [-3.0, np.nan]], dtype=np.float32)
    idx = np.array([[0, 1], [0, 2], [0, -1], [0, 99], [1, 1]])
    ref = R.neighbor_maxpool_ref(x, idx)
    # below 0, N and above N all mean the zero row; a NaN is skipped, all-NaN gives -inf
    want = np.array([[-1.0, 2.0], [0.0, 2.0], [0.0, 2.0], [0.0, 2.0], [-3.0, -np.inf]], dtype=np.float32)
    assert np.array_equal(ref, want)
