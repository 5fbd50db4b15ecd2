"""In-tree build of ``libopenprovence_hip.so`` with hipcc for gfx950 (cross-compiles without a GPU).

The library is several translation units -- the C ABI plus one unit per kernel family, each instantiating its
templates for every curated precision policy -- compiled in parallel into ``build/`` and linked into one shared
object next to the package.
"""

from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
INCLUDE = PKG_DIR.parent / "include" / "open_provence_hip.h"
BUILD_DIR = PKG_DIR.parent / "build" / "hip"
OUTPUT = PKG_DIR / "libopenprovence_hip.so"

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.MULTILINE)


def scan_includes(src: Path) -> list[Path]:
    """Every file ``src`` reaches through quoted ``#include "..."`` lines, transitively (headers, ``.inc`` bodies and the C
    header alike), each name resolved against the including file's directory.  A name that resolves to no file is listed too."""

    found: set[Path] = set()
    todo = [src]
    while todo:
        path = todo.pop()
        for name in _INCLUDE.findall(path.read_text()):
            inc = Path(os.path.normpath(path.parent / name))
            if inc not in found:
                found.add(inc)
                if inc.is_file():
                    todo.append(inc)
    return sorted(found)


# (object name, source, extra defines); what an object depends on beside its source is scanned from the source (scan_includes)
UNITS = [
    # the C ABI, cut by concern; op_handle.h is what they share
    ("op_api", CSRC / "op_api.hip", []),
    ("op_weights", CSRC / "op_weights.hip", []),
    ("op_select", CSRC / "op_select.hip", []),
    ("op_forward", CSRC / "op_forward.hip", []),
    ("op_forward_layers", CSRC / "op_forward_layers.hip", []),
    ("op_forward_masked", CSRC / "op_forward_masked.hip", []),
    ("op_attention_side", CSRC / "op_attention_side.hip", []),
    ("op_services", CSRC / "op_services.hip", []),
    # one launch unit per kernel family
    ("op_launch_row0", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=0"]),
    ("op_launch_row1", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=1"]),
    ("op_launch_row2", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=2"]),
    ("op_launch_row3", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=3"]),
    ("op_launch_row4", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=4"]),
    ("op_launch_row5", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=5"]),
    ("op_launch_row6", CSRC / "op_launch_row.hip", ["-DOPL_ROW_PART=6"]),
    ("op_launch_layer32", CSRC / "op_launch_layer32.hip", []),
    ("op_launch_attn", CSRC / "op_launch_attn.hip", []),
    ("op_launch_attn_masked", CSRC / "op_launch_attn_masked.hip", []),
    ("op_launch_panel", CSRC / "op_launch_panel.hip", []),
    ("op_launch_padded", CSRC / "op_launch_padded.hip", []),
    ("op_launch_audit", CSRC / "op_launch_audit.hip", []),
    ("op_launch_f32", CSRC / "op_launch_f32.hip", []),
    ("op_launch_f32_masked", CSRC / "op_launch_f32_masked.hip", []),
    ("op_launch_attn_probs", CSRC / "op_launch_attn_probs.hip", []),
    ("op_launch_probe", CSRC / "op_launch_probe.hip", []),
    ("op_launch_loss", CSRC / "op_launch_loss.hip", []),
    ("op_launch_assemble", CSRC / "op_launch_assemble.hip", []),
    ("op_launch_decide", CSRC / "op_launch_decide.hip", []),
]
SOURCES = sorted({u[1] for u in UNITS})
HEADERS = sorted({h for src in SOURCES for h in scan_includes(src)})

FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-Wno-unused-result",
    # no SLP vectorizer: it fuses adjacent scalar fp32 ops of the epilogues into v_pk_* instructions, which cost
    # more issue time beside MFMAs than the two scalar ops they replace (measured: +1.1 % pairs/s without it)
    "-fno-slp-vectorize",
]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, PATH and /opt/rocm/bin/hipcc)")


def _unit_digest(unit) -> str:
    _, src, defines = unit
    digest = hashlib.sha256(" ".join(FLAGS + defines).encode())
    for path in [src, *scan_includes(src)]:
        digest.update(path.read_bytes())
    return digest.hexdigest()


def _unit_is_stale(unit) -> bool:
    obj = BUILD_DIR / f"{unit[0]}.o"
    stamp = BUILD_DIR / f"{unit[0]}.sha256"
    return not (obj.exists() and stamp.exists() and stamp.read_text() == _unit_digest(unit))


def is_stale() -> bool:
    if not OUTPUT.exists():
        return True
    built = OUTPUT.stat().st_mtime
    return any(p.stat().st_mtime > built for p in SOURCES + HEADERS)


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile every HIP source into the shared library next to the package; returns its path."""

    if not force and not is_stale():
        return OUTPUT
    hipcc = _hipcc()
    BUILD_DIR.mkdir(parents=True, exist_ok=True)

    def compile_unit(unit) -> None:
        name, src, defines = unit
        obj = BUILD_DIR / f"{name}.o"
        cmd = [hipcc, *FLAGS, *defines, "-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd), flush=True)
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src.name} {defines} ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
        (BUILD_DIR / f"{name}.sha256").write_text(_unit_digest(unit))

    todo = [u for u in UNITS if force or _unit_is_stale(u)]
    # MAX_JOBS where it is set; else the CPUs, but at most 16: a shared machine shows many times what one command may use
    max_jobs = os.environ.get("MAX_JOBS", "").strip()
    jobs = int(max_jobs) if max_jobs.isdigit() and int(max_jobs) > 0 else min(os.cpu_count() or 4, 16)
    with ThreadPoolExecutor(max_workers=max(1, min(len(todo), jobs))) as pool:
        list(pool.map(compile_unit, todo))
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(OUTPUT), *[str(BUILD_DIR / f"{u[0]}.o") for u in UNITS]]
    if verbose:
        print(" ".join(link), flush=True)
    proc = subprocess.run(link, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"link failed ({proc.returncode}):\n{proc.stdout}\n{proc.stderr}")
    return OUTPUT


if __name__ == "__main__":
    print(build(force=True, verbose=True))
