"""One definition of the shared device helpers (no GPU, no build: reads the files).

A forward and its backward must draw the same dropout mask, and one training step mixes kernels
from several translation units, so `drop_scale`, the float4 helpers and the device work-item
struct are defined once, in csrc/ppgat_device.h, which the .hip files include.  These checks
keep a copy from growing back.  csrc/lab/ is not read.
"""
from __future__ import annotations

import functools
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parents[1] / "plotpointe-gat-recommendation_amd" / "csrc"
LAB = CSRC / "lab"
HEADER = "ppgat_device.h"

# helper name -> return type of the shared definition.  The type is part of the pattern for one
# reason: ppgat::split::absmax4 (ppgat_split.h) is another function -- float absmax4(const
# float4&), the largest |component| of one vector -- that exists once and stays where it is.
HELPERS = {
    "ld4": "float4", "st4": "void", "f4": "float4", "fma4": "float4", "add4": "float4", "mul4": "float4",
    "dot4": "float", "comp": "float", "shfl_xor4": "float4", "absmax4": "float4", "colmax_merge4": "void",
    "ld4s": "float4", "st4s": "void", "lrelu": "float", "dlrelu": "float", "drop_scale": "float",
    "clamp_idx": "int64_t",
}
# the one overload that stays local: ld4 of a global-address-space pointer (ppgat_gemm.hip)
LOCAL_OVERLOADS = {("ppgat_gemm.hip", "ld4"): r"\(\s*gfloat\s*\*"}


@functools.lru_cache(maxsize=None)
def _sources() -> dict[str, str]:
    files = [p for p in CSRC.rglob("*") if p.suffix in (".hip", ".h", ".cpp") and LAB not in p.parents
             and "build" not in p.relative_to(CSRC).parts]
    assert len(files) >= 15, files  # the translation units and their headers were found
    return {p.name: p.read_text() for p in sorted(files)}


def _definitions(text: str, name: str, ret: str) -> list[str]:
    """The parameter lists of the definitions `ret name(...) {` in text."""
    return [m.group(1) for m in re.finditer(rf"\b{ret}\s+{name}\s*(\([^;{{}}]*\))\s*\{{", text)]


@pytest.mark.parametrize("name", sorted(HELPERS))
def test_helper_is_defined_once_in_the_device_header(name):
    where = []
    for fname, text in _sources().items():
        for params in _definitions(text, name, HELPERS[name]):
            local = LOCAL_OVERLOADS.get((fname, name))
            if local and re.match(local, params):
                continue
            where.append(fname)
    assert where == [HEADER], (name, where)


def test_items_struct_is_defined_once_in_the_device_header():
    where = [fname for fname, text in _sources().items() for _ in re.finditer(r"\bstruct\s+Items\b\s*\{", text)]
    assert where == [HEADER], where


def test_the_retired_item_structs_are_gone():
    for fname, text in _sources().items():
        assert not re.search(r"\bstruct\s+(XItems|ItemsArg)\b", text), fname


def test_the_local_overload_pattern_still_matches_something():
    # the exemption above must not outlive the overload it was written for
    text = _sources()["ppgat_gemm.hip"]
    assert [p for p in _definitions(text, "ld4", "float4") if re.match(LOCAL_OVERLOADS[("ppgat_gemm.hip", "ld4")], p)]
