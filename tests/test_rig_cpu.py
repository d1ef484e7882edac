"""Rig submissions (one cloud under C images per forward), the parts that need no GPU: the two entry points are declared in
include/cofi_hip.h and mirrored by the ctypes table, the ABI version did not move, and FrameBatcher refuses a batch that is no whole
number of rigs before it touches the model."""
import ctypes

import pytest

from cofii2p_amd import _lib


def test_header_declares_the_rig_entry_points():
    syms = _lib.header_symbols()
    assert "cofi_repeat_frames" in syms
    assert "cofi_match_finish_rig" in syms


def test_header_and_binding_table_name_the_same_functions():
    assert set(_lib.header_symbols()) == set(_lib.SIGNATURES)


def test_match_finish_rig_is_match_finish_plus_one_int():
    res, args = _lib.SIGNATURES["cofi_match_finish"]
    res_rig, args_rig = _lib.SIGNATURES["cofi_match_finish_rig"]
    assert res_rig is res
    assert len(args_rig) == len(args) + 1
    assert args_rig.count(ctypes.c_int) == args.count(ctypes.c_int) + 1
    for t in (ctypes.c_void_p, ctypes.c_float):
        assert args_rig.count(t) == args.count(t)
    # the divisor sits between `frames` and the stream
    assert args_rig[:-2] == args[:-1] and args_rig[-2] is ctypes.c_int and args_rig[-1] is args[-1]


def test_repeat_frames_signature():
    res, args = _lib.SIGNATURES["cofi_repeat_frames"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, I, I, I, I, I, P, I, P]   # src, lds, rows_per_frame, cols, frames, times, dst, ldd, stream


def test_abi_version_did_not_move():
    assert _lib.ABI_VERSION == 3


def test_frame_batcher_refuses_a_batch_that_is_no_whole_number_of_rigs():
    from cofii2p_amd.serving import FrameBatcher

    with pytest.raises(ValueError):
        FrameBatcher(None, batch=16, cameras=3)   # raised before the model (None here) is touched
    with pytest.raises(ValueError):
        FrameBatcher(None, batch=16, cameras=0)
