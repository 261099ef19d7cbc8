"""Camera-subset sweeps, the parts that need no GPU: the subset tables (handmvnet_amd/subsets.py), the by-count averaging and the
new entry's place in the C ABI."""
import math
import os
import re

import numpy as np
import pytest
import torch

from handmvnet_amd import _lib
from handmvnet_amd.subsets import as_subset_table, by_count, k_of_n, subset_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k_of_n_counts_and_order():
    for V in range(1, 9):
        for k in range(1, V + 1):
            subs = k_of_n(V, k)
            assert len(subs) == math.comb(V, k)
            assert all(len(s) == k and s == sorted(set(s)) and 0 <= s[0] and s[-1] < V for s in subs)
            assert subs == sorted(subs) and len({tuple(s) for s in subs}) == len(subs)      # lexicographic, no repeats
    assert k_of_n(4, 2) == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert len(k_of_n(8, 4)) == 70 and k_of_n(8, 4)[0] == [0, 1, 2, 3] and k_of_n(8, 4)[-1] == [4, 5, 6, 7]
    for V, k in ((4, 0), (4, 5), (0, 1)):
        with pytest.raises(ValueError):
            k_of_n(V, k)
    import handmvnet_amd
    assert handmvnet_amd.k_of_n is k_of_n and handmvnet_amd.as_subset_table is as_subset_table      # the package's lazy exports
    assert handmvnet_amd.SubsetSweepEvaluator.__name__ == "SubsetSweepEvaluator"


def test_as_subset_table_accepts_masks_and_index_lists():
    want = np.array([[1, 0, 1, 0], [0, 0, 0, 1], [1, 1, 1, 1], [1, 0, 1, 0]], dtype=np.uint8)
    lists = [[0, 2], [3], [0, 1, 2, 3], [2, 0]]      # (any order inside a list; a duplicate subset is allowed)
    for given in (lists, [tuple(s) for s in lists], [np.array(s) for s in lists], want.astype(bool), want, want.astype(bool).tolist(),
                  torch.from_numpy(want.astype(bool)), want.astype(np.int64)):
        t = as_subset_table(given, 4)
        assert t.dtype == np.uint8 and t.flags["C_CONTIGUOUS"] and np.array_equal(t, want)
    assert subset_lists(want) == [[0, 2], [3], [0, 1, 2, 3], [0, 2]]
    assert np.array_equal(as_subset_table(k_of_n(8, 4), 8).sum(axis=1), np.full(70, 4))


def test_as_subset_table_refuses_bad_subsets():
    with pytest.raises(ValueError, match="no camera"):
        as_subset_table([[0, 1], []], 4)
    with pytest.raises(ValueError, match="no camera"):
        as_subset_table(np.array([[True, False], [False, False]]), 2)
    with pytest.raises(ValueError, match="outside"):
        as_subset_table([[0, 4]], 4)
    with pytest.raises(ValueError, match="outside"):
        as_subset_table([[-1]], 4)
    with pytest.raises(ValueError, match="twice"):
        as_subset_table([[1, 1]], 4)
    with pytest.raises(ValueError, match="columns"):
        as_subset_table(np.ones((2, 5), dtype=bool), 4)      # a wrong V
    with pytest.raises(ValueError, match="columns"):
        as_subset_table([[True, False, True]], 4)
    with pytest.raises(ValueError, match="at least one subset"):
        as_subset_table([], 4)
    with pytest.raises(ValueError):
        as_subset_table(np.ones(4, dtype=bool), 4)           # one row is not a table


def test_new_entry_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    assert re.search(r"\bint\s+hmv_forward_subsets\s*\(", header)
    lib = _lib.load()
    assert hasattr(lib, "hmv_forward_subsets") and "hmv_forward_subsets" in _lib.SYMBOLS
    assert len(lib.hmv_forward_subsets.argtypes) == 11
    # a null handle is refused before anything touches HIP
    assert lib.hmv_forward_subsets(None, 1, 1, None, None, None, None, None, None, None, None) != 0


def test_by_count_is_the_plain_mean_per_view_count():
    subsets = [[0], [1, 2], [0, 2], [3], [0, 1, 2]]
    per = [{"test_mpjpe": 10.0, "test/loss": 1.0, "test_pck_j": [0.1, 0.2], "samples": 8},
           {"test_mpjpe": 4.0, "test/loss": None, "test_pck_j": [0.3, 0.4], "samples": 8},
           {"test_mpjpe": 6.0, "test/loss": 2.0, "test_pck_j": [0.5, 0.6], "samples": 8},
           {"test_mpjpe": 20.0, "test/loss": 3.0, "test_pck_j": [0.7, 0.8], "samples": 8},
           {"test_mpjpe": 1.0, "test/loss": 0.5, "test_pck_j": [0.9, 1.0], "samples": 8}]
    got = by_count(per, subsets)
    assert sorted(got) == [1, 2, 3]
    assert got[1] == {"test_mpjpe": 15.0, "test/loss": 2.0, "samples": 8.0, "subsets": 2}
    assert got[2] == {"test_mpjpe": 5.0, "test/loss": None, "samples": 8.0, "subsets": 2}      # a loss one of the subsets lacks is None
    assert got[3] == {"test_mpjpe": 1.0, "test/loss": 0.5, "samples": 8.0, "subsets": 1}
    with pytest.raises(ValueError):
        by_count(per[:2], subsets)
