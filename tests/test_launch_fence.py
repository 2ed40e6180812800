"""The launch fence of the Python package (no GPU, no build: reads the files).

The GAT layers' kernels are launched from _launch.py alone: row offsets become addresses in
_lib.row_ptr, and dist.py -- exchanges, phases, streams -- never touches the C ABI itself.
"""
from __future__ import annotations

import ast
import re
from importlib import import_module
from pathlib import Path

PKG = Path(__file__).resolve().parents[1] / "plotpointe-gat-recommendation_amd"


def test_dist_does_not_touch_the_abi():
    tree = ast.parse((PKG / "dist.py").read_text())
    imported = {a.name.split(".")[0] for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    imported |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) and n.level == 0}
    assert "ctypes" not in imported
    assert "lib.ppgat_" not in (PKG / "dist.py").read_text()


def test_pointer_arithmetic_lives_in_the_launch_layer():
    files = sorted(PKG.glob("*.py"))
    assert len(files) >= 15, files
    found = [(p.name, n) for p in files if p.name not in ("_lib.py", "_launch.py")
             for n, line in enumerate(p.read_text().splitlines(), 1) if re.search(r"data_ptr\(\)\s*\+", line)]
    assert not found, found


def test_launch_layer_calls_declared_entries_only():
    sigs = import_module("plotpointe-gat-recommendation_amd._lib").SIGNATURES
    called = set(re.findall(r"\.(ppgat_\w+)\b", (PKG / "_launch.py").read_text()))
    assert len(called) >= 25, called  # the entries and their workspace queries were found
    assert called <= set(sigs), called - set(sigs)
