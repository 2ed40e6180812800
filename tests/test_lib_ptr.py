"""The pointer helpers every kernel launch goes through (_lib.row_ptr, seed64, edge_ptrs): host
only, on CPU tensors (data_ptr() works on them)."""
from __future__ import annotations

from importlib import import_module

import pytest
import torch

_lib = import_module("plotpointe-gat-recommendation_amd._lib")


def test_row_ptr_rows_of_a_matrix():
    t = torch.zeros(5, 3, dtype=torch.float32)
    base = t.data_ptr()
    assert _lib.row_ptr(t) == (base, 3)
    assert _lib.row_ptr(t, 0) == (base, 3)
    assert _lib.row_ptr(t, 2) == (base + 24, 3)
    # one past the end (a zero-row range): the address, not the null pointer of the empty slice
    assert _lib.row_ptr(t, 5) == (base + 60, 3)
    assert t[5:].numel() == 0


def test_row_ptr_inner_dimensions_and_element_size():
    t = torch.zeros(6, 2, 4, dtype=torch.float32)
    assert _lib.row_ptr(t, 3) == (t.data_ptr() + 96, 8)
    i = torch.zeros(9, dtype=torch.int32)
    assert _lib.row_ptr(i, 4) == (i.data_ptr() + 16, 1)
    w = torch.zeros(4, 3, dtype=torch.int64)
    assert _lib.row_ptr(w, 2) == (w.data_ptr() + 48, 3)


def test_row_ptr_column_view():
    S = torch.zeros(7, 8, dtype=torch.float32)
    assert _lib.row_ptr(S[:, 4:]) == (S.data_ptr() + 16, 8)
    assert _lib.row_ptr(S[:, 4:], 2) == (S.data_ptr() + 16 + 64, 8)


def test_row_ptr_none():
    assert _lib.row_ptr(None) == (None, 0)
    assert _lib.row_ptr(None, 3) == (None, 0)


def test_row_ptr_rejects_rows_outside_and_gapped_rows():
    t = torch.zeros(5, 3, dtype=torch.float32)
    with pytest.raises(IndexError):
        _lib.row_ptr(t, 6)
    with pytest.raises(IndexError):
        _lib.row_ptr(t, -1)
    with pytest.raises(ValueError):
        _lib.row_ptr(t.t())
    with pytest.raises(ValueError):
        _lib.row_ptr(torch.zeros(4, 3, 6)[:, :, :5])


def test_seed64():
    assert _lib.seed64(-1) == 2**64 - 1
    assert _lib.seed64(7) == 7
    assert _lib.seed64(2**64 + 3) == 3


def test_edge_ptrs():
    a, b = torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)
    assert _lib.edge_ptrs(4, a, b, None) == (a.data_ptr(), b.data_ptr(), None)
    assert _lib.edge_ptrs(0, a, b, None) == (None, None, None)
    assert _lib.edge_ptrs(0) == ()
