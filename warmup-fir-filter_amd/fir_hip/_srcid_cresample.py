"""The source id of libfir_cresample.so: a hash of the sources it is built from.

``make -C warmup-fir-filter_amd/csrc_cresample`` embeds it (``-DFIR_CRESAMPLE_BUILD_ID``, exported as
``fir_cresample_build_id()``); :func:`fir_hip.cresample.lib` recomputes it from the sources beside the
package and refuses a library built from other sources.  The sources are everything in
``csrc_cresample/``, its header, and the headers it includes from the first library: the two
header-only device helpers of ``csrc/`` and ``include/fir_hip.h`` (the status and stage values).
Standalone on purpose (no NumPy, no import of the package): the Makefile runs it as
``python3 _srcid_cresample.py``.
"""
from __future__ import annotations

import hashlib
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parents[1]  # warmup-fir-filter_amd/
SHARED_HEADERS = ("fir_common.h", "fir_dispatch.h")  # of csrc/


def source_files(pkg: Path = PKG) -> list[Path]:
    own = pkg / "csrc_cresample"
    files = sorted(p for p in own.iterdir() if p.is_file() and p.suffix in (".hip", ".h")) if own.is_dir() else []
    files += [own / "Makefile", pkg.parent / "include" / "fir_cresample.h", pkg.parent / "include" / "fir_hip.h"]
    files += [pkg / "csrc" / name for name in SHARED_HEADERS]
    return files


def source_id(pkg: Path = PKG) -> str | None:
    """sha256 over (path relative to the repo root, contents) of every source; None when the
    sources are not present (a library used without its tree)."""
    files = source_files(pkg)
    if not all(p.is_file() for p in files):
        return None
    h = hashlib.sha256()
    for p in files:
        h.update(p.relative_to(pkg.parent).as_posix().encode() + b"\0")
        h.update(p.read_bytes() + b"\0")
    return h.hexdigest()[:32]


if __name__ == "__main__":
    sid = source_id()
    if sid is None:
        sys.exit("libfir_cresample sources not found")
    print(sid)
