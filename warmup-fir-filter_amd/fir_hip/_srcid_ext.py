"""The source id of an extension library (libfir_cdecim.so, libfir_cinterp.so, libfir_cresample.so,
libfir_cstream.so, libfir_crstream.so): a hash of the sources it is built from.

``make -C warmup-fir-filter_amd/csrc_<name>`` embeds it (``-DFIR_<NAME>_BUILD_ID``, exported as
``fir_<name>_build_id()``); the loader (:mod:`fir_hip._ext`) recomputes it from the sources beside
the package and refuses a library built from other sources.  The sources are everything in
``csrc_<name>/``, its header, the headers it includes from the first library (the two header-only
device helpers of ``csrc/`` and ``include/fir_hip.h``, the status and stage values) and every file
of ``csrc_cext/``, the host layer, the device header (``cext_device.h``) and the make rules the
extension libraries share.
Standalone on purpose (no NumPy, no import of the package): the make rules run it as
``python3 _srcid_ext.py <name>``.
"""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parents[1]  # warmup-fir-filter_amd/
SHARED_HEADERS = ("fir_common.h", "fir_dispatch.h")  # of csrc/
SHARED_DIR = "csrc_cext"


def source_files(name: str, pkg: Path = PKG) -> list[Path]:
    own, shared = pkg / f"csrc_{name}", pkg / SHARED_DIR
    files = sorted(p for p in own.iterdir() if p.is_file() and p.suffix in (".hip", ".h")) if own.is_dir() else []
    files += [own / "Makefile", pkg.parent / "include" / f"fir_{name}.h", pkg.parent / "include" / "fir_hip.h"]
    files += [pkg / "csrc" / header for header in SHARED_HEADERS]
    # a missing shared directory stands for itself: not a file, so source_id gives None
    files += sorted(p for p in shared.iterdir() if p.is_file()) if shared.is_dir() else [shared]
    return files


def source_id(name: str, pkg: Path = PKG) -> str | None:
    """sha256 over (path relative to the repo root, contents) of every source; None when the
    sources are not present (a library used without its tree)."""
    files = source_files(name, pkg)
    if not all(p.is_file() for p in files):
        return None
    h = hashlib.sha256()
    for p in files:
        h.update(p.relative_to(pkg.parent).as_posix().encode() + b"\0")
        h.update(p.read_bytes() + b"\0")
    return h.hexdigest()[:32]


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: _srcid_ext.py <name>   (cdecim, cinterp, cresample, cstream or crstream)")
    sid = source_id(sys.argv[1])
    if sid is None:
        sys.exit(f"libfir_{sys.argv[1]} sources not found")
    print(sid)
