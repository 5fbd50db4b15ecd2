"""The build description (``open_provence_amd/build_ext.py``): its units cover every source, what an object depends on is
scanned from the ``#include`` lines, and no kernel is compiled into two objects.

Needs no device and no compiler: the sources are read as text.

One definition per kernel.  A non-template ``__global__`` function has external linkage, so a header that defines one must be
compiled into exactly one unit; a template kernel may sit in a shared header (it is instantiated where it is launched).  A
kernel inside ``#ifdef NAME ... #endif`` counts for the units that define NAME (``#define`` in the source, ``-DNAME`` in the
unit's defines) -- the pack kernels behind OPK_PACK_KERNELS, the fp32 kernels behind OPK_F32_KERNELS."""

from __future__ import annotations

import re
import shutil
from pathlib import Path

import pytest

from open_provence_amd import build_ext

_DIRECTIVE = re.compile(r"^[ \t]*#[ \t]*(ifdef|ifndef|if|elif|else|endif)\b[ \t]*(\w*)")


def _kernels(path: Path) -> list[tuple[str, bool, frozenset]]:
    """(name, is_template, the ``#ifdef`` names around it) of every ``__global__`` function ``path`` defines."""

    out, guards, last_code = [], [], ""
    for line in path.read_text().splitlines():
        directive = _DIRECTIVE.match(line)
        if directive:
            kind, name = directive.groups()
            if kind in ("ifdef", "ifndef", "if"):
                guards.append(name if kind == "ifdef" else None)  # (#if / #ifndef: counted as always compiled)
            elif kind in ("elif", "else"):
                guards[-1] = None
            else:
                guards.pop()
            continue
        code = line.split("//")[0].strip()
        if "__global__" in code:
            name = re.search(r"\bvoid\s+(\w+)\s*\(", code)
            assert name, f"{path.name}: cannot read the kernel's name from {line!r}"
            out.append((name.group(1), last_code.startswith("template"), frozenset(g for g in guards if g)))
        if code and not code.startswith("#"):
            last_code = code
    assert not guards, f"{path.name}: unbalanced #if / #endif"
    return out


def _defined(unit) -> set[str]:
    """The macros a unit defines for its headers: ``#define`` lines of its source, ``-D`` of its defines."""

    _, src, defines = unit
    names = set(re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)", src.read_text(), flags=re.M))
    return names | {d[2:].split("=")[0] for d in defines if d.startswith("-D")}


def test_every_source_is_a_unit():
    sources = {u[1] for u in build_ext.UNITS}
    assert sorted(build_ext.CSRC.glob("*.hip")) == sorted(sources)
    names = [u[0] for u in build_ext.UNITS]
    assert len(set(names)) == len(names), "two units would write the same object"
    assert len({(u[1], tuple(u[2])) for u in build_ext.UNITS}) == len(names), "the same source with the same defines twice"


def test_every_scanned_file_exists():
    for _, src, _ in build_ext.UNITS:
        found = build_ext.scan_includes(src)
        assert found, src
        for path in found:
            assert path.is_file(), f"{src.name} includes {path}, which does not exist"
    # the scan follows .inc bodies and the C header, and resolves against the including file's directory
    row = {p.name for p in build_ext.scan_includes(build_ext.CSRC / "op_launch_row.hip")}
    assert {"open_provence_hip.h", "op_internal.h", "opk_rowgemm_mlp_loop.inc", "opk_layer16p_body.inc"} <= row
    assert build_ext.INCLUDE in build_ext.HEADERS
    assert all(h.suffix != ".hip" for h in build_ext.HEADERS)


def test_a_units_digest_follows_every_header_it_reaches(tmp_path, monkeypatch):
    csrc = tmp_path / "open_provence_amd" / "csrc"
    shutil.copytree(build_ext.CSRC, csrc)
    (tmp_path / "include").mkdir()
    shutil.copy(build_ext.INCLUDE, tmp_path / "include" / build_ext.INCLUDE.name)
    units = [(name, csrc / src.name, defines) for name, src, defines in build_ext.UNITS]
    monkeypatch.setattr(build_ext, "CSRC", csrc)
    monkeypatch.setattr(build_ext, "INCLUDE", tmp_path / "include" / build_ext.INCLUDE.name)
    monkeypatch.setattr(build_ext, "UNITS", units)

    reach = {u[0]: set(build_ext.scan_includes(u[1])) for u in units}
    assert all(str(p).startswith(str(tmp_path)) for found in reach.values() for p in found), "the scan left the copied tree"
    before = {u[0]: build_ext._unit_digest(u) for u in units}
    for header in sorted(set().union(*reach.values())):
        original = header.read_bytes()
        header.write_bytes(original + b"\n// changed\n")
        for u in units:
            changed = build_ext._unit_digest(u) != before[u[0]]
            assert changed == (header in reach[u[0]]), f"{u[0]} after a change of {header.name}: digest changed = {changed}"
        header.write_bytes(original)
    assert {u[0]: build_ext._unit_digest(u) for u in units} == before
    # ... and its own source, and its defines
    name, src, defines = units[0]
    assert build_ext._unit_digest((name, src, defines + ["-DX=1"])) != before[name]
    src.write_bytes(src.read_bytes() + b"\n")
    assert build_ext._unit_digest(units[0]) != before[name]


def test_no_kernel_is_compiled_into_two_units():
    compiled: dict[tuple[str, str], list[str]] = {}
    for unit in build_ext.UNITS:
        defined = _defined(unit)
        for header in [unit[1], *build_ext.scan_includes(unit[1])]:
            for name, is_template, guards in _kernels(header):
                if not is_template and guards <= defined:
                    compiled.setdefault((header.name, name), []).append(unit[0])
    assert compiled, "found no kernel at all"
    twice = {k: v for k, v in compiled.items() if len(v) > 1}
    assert not twice, f"non-template kernels compiled into more than one unit: {twice}"
    # the weight packs: behind OPK_PACK_KERNELS, which one unit defines
    assert [u[0] for u in build_ext.UNITS if "OPK_PACK_KERNELS" in _defined(u)] == ["op_weights"]
    assert compiled[("opk_panel.hip.h", "pack_panel_kernel")] == ["op_weights"]


def test_shared_kernel_family_headers_hold_templates_only():
    # op_internal.h includes the kernel families' headers for their parameter structs, so every unit reaches them: outside an
    # #ifdef that one unit switches on, their kernels are templates
    shared = build_ext.scan_includes(build_ext.CSRC / "op_internal.h")
    assert {"opk_panel.hip.h", "opk_rowgemm.hip.h", "opk_attn.hip.h", "opk_f32.hip.h"} <= {p.name for p in shared}
    n = 0
    for header in shared:
        for name, is_template, guards in _kernels(header):
            n += 1
            assert is_template or guards, f"{header.name}: {name} is neither a template nor behind an #ifdef, and every unit includes it"
    assert n > 10
