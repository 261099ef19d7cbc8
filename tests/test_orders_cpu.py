"""Reference-view sweeps without a GPU: the order tables (handmvnet_amd/orders.py), the two new entries in the header, the library
and the binding, and every refusal of hmv_op_pose_consensus, which comes before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from handmvnet_amd import _lib
from handmvnet_amd.orders import as_order_table, each_reference, order_lists, rotations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_as_order_table_accepts():
    t = as_order_table([[2, 0, 1], [3], [1, 0]], 4)
    assert t.dtype == np.int32 and t.flags["C_CONTIGUOUS"]
    assert t.tolist() == [[2, 0, 1, -1], [3, -1, -1, -1], [1, 0, -1, -1]]
    assert order_lists(t) == [[2, 0, 1], [3], [1, 0]]
    # a padded table (array or tensor) passes through; duplicates are allowed; a narrower table is widened
    assert as_order_table(t, 4).tobytes() == t.tobytes()
    assert as_order_table(torch.from_numpy(t), 4).tobytes() == t.tobytes()
    assert as_order_table(np.array([[1, 0], [1, 0]]), 3).tolist() == [[1, 0, -1], [1, 0, -1]]
    assert as_order_table([(0, 1, 2, 3)], 4).tolist() == [[0, 1, 2, 3]]
    assert as_order_table([np.array([1, 0]), torch.tensor([2])], 3).tolist() == [[1, 0, -1], [2, -1, -1]]
    assert as_order_table([[0]], 1).tolist() == [[0]]


@pytest.mark.parametrize("orders, V, text", [
    ([], 4, "at least one order"),
    ([[0, 1], []], 4, "no camera"),
    ([[-1, -1, -1, -1]], 4, "no camera"),
    ([[0, 4]], 4, r"outside \[0, 4\)"),
    ([[0, -2]], 4, r"outside \[0, 4\)"),
    ([[1, 2, 1]], 4, "named twice"),
    ([[0, -1, 2, -1]], 4, "after a -1"),
    ([[0, 1, 2, 3, 0]], 4, "4 cameras"),
    ([[0.5, 1]], 4, "integers"),
    ([[True, False]], 4, "integers"),
    (np.zeros((1, 2)), 4, "sequence of camera-index lists"),
    (np.zeros(3, dtype=np.int32), 4, "sequence of camera-index lists"),
])
def test_as_order_table_refuses(orders, V, text):
    with pytest.raises(ValueError, match=text):
        as_order_table(orders, V)


def test_each_reference_and_rotations():
    assert each_reference(4) == [[0, 1, 2, 3], [1, 0, 2, 3], [2, 0, 1, 3], [3, 0, 1, 2]]
    assert rotations(4) == [[0, 1, 2, 3], [1, 2, 3, 0], [2, 3, 0, 1], [3, 0, 1, 2]]
    assert each_reference(1) == rotations(1) == [[0]]
    for V in (1, 2, 7, 8):
        for orders in (each_reference(V), rotations(V)):
            assert len(orders) == V and [o[0] for o in orders] == list(range(V))
            assert all(sorted(o) == list(range(V)) for o in orders)
            assert as_order_table(orders, V).shape == (V, V)
        assert all(o[1:] == sorted(o[1:]) for o in each_reference(V))
    for f in (each_reference, rotations):
        with pytest.raises(ValueError):
            f(0)


def test_new_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    assert re.search(r"\bint\s+hmv_forward_orders\s*\(", header)
    assert re.search(r"\bint\s+hmv_op_pose_consensus\s*\(", header)
    assert re.search(r"\}\s*hmv_consensus_args\s*;", header)
    lib = _lib.load()
    for name in ("hmv_forward_orders", "hmv_op_pose_consensus"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert len(lib.hmv_forward_orders.argtypes) == 11
    assert len(lib.hmv_op_pose_consensus.argtypes) == 3
    # 8 int32 fields and 7 pointers, as the header lays them out
    assert ctypes.sizeof(_lib.HmvConsensusArgs) == 8 * 4 + 7 * ctypes.sizeof(ctypes.c_void_p)
    fields = re.search(r"typedef struct hmv_consensus_args \{(.*?)\} hmv_consensus_args;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*(?=[,;])", fields)
    assert names == [f[0] for f in _lib.HmvConsensusArgs._fields_]
    # a null handle is refused before anything touches HIP
    assert lib.hmv_forward_orders(None, 1, 1, None, None, None, None, None, None, None, None) != 0


def _args(**over):
    """A well-formed argument struct on fake non-null addresses: every refusal comes before the first HIP call, so none is read."""
    a = _lib.HmvConsensusArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvConsensusArgs)
    a.S, a.B, a.V, a.target_cam, a.mode, a.iterations = 3, 2, 4, 1, 0, 16
    a.poses, a.ref_cam, a.extrinsic = 0x1000, 0x2000, 0x3000
    a.aligned, a.consensus, a.spread, a.deviation = 0x4000, 0x5000, 0x6000, 0x7000
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over, text", [
    (dict(S=0), b"S must"), (dict(B=0), b"B must"), (dict(V=0), b"V must"), (dict(S=-1), b"S must"),
    (dict(target_cam=-1), b"target_cam"), (dict(target_cam=4), b"target_cam"),
    (dict(poses=None), b"poses"), (dict(ref_cam=None), b"ref_cam"), (dict(extrinsic=None), b"extrinsic"),
    (dict(aligned=None, consensus=None, spread=None, deviation=None), b"every output is NULL"),
    (dict(struct_size=ctypes.sizeof(_lib.HmvConsensusArgs) - 8), b"struct_size"), (dict(struct_size=0), b"struct_size"),
    (dict(iterations=-1), b"iterations"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
])
def test_pose_consensus_refuses_bad_arguments_without_a_device(over, text):
    lib = _lib.load()
    rc = lib.hmv_op_pose_consensus(0, ctypes.byref(_args(**over)), None)
    msg = lib.hmv_last_error(None)
    assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_op_pose_consensus" in msg and text in msg, (over, rc, msg)


def test_pose_consensus_refuses_null_args():
    lib = _lib.load()
    assert lib.hmv_op_pose_consensus(0, None, None) == _lib.HMV_ERR_ARG
    assert b"args is NULL" in lib.hmv_last_error(None)


def test_pose_consensus_python_refusals_come_before_the_library():
    from handmvnet_amd.orders import pose_consensus
    with pytest.raises(ValueError, match="mode"):
        pose_consensus(torch.zeros(2, 1, 21, 3), [0, 1], torch.zeros(1, 2, 4, 4), mode="mode")
    with pytest.raises(ValueError, match=r"\[S, B, 21, 3\]"):
        pose_consensus(torch.zeros(2, 21, 3), [0, 1], torch.zeros(1, 2, 4, 4))
    with pytest.raises(_lib.HandMvError, match="no CPU fallback"):
        pose_consensus(torch.zeros(2, 1, 21, 3), [0, 1], torch.zeros(1, 2, 4, 4))
