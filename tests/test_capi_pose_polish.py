"""The Python / C boundary of include/posecnn_hip/pose_polish.h (CPU only): what tests/test_capi_bindings.py holds every
header of include/*.h to, for the one header that lives in a subdirectory — bound as declared, its exact symbol list,
self-contained, no ABI version of its own, every symbol exported and at home in one header."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "posecnn_hip/pose_polish.h"
PINNED = ["pcnn_pose2d_estimate_polished_fwd", "pcnn_pose2d_estimate_polished_workspace_bytes", "pcnn_pose3d_estimate_polished_fwd",
          "pcnn_pose3d_estimate_polished_workspace_bytes", "pcnn_pose_polish_fwd", "pcnn_pose_polish_workspace_bytes"]


@pytest.fixture(scope="module")
def L():
    from posecnn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_header_is_bound_as_declared(L):
    from posecnn_amd import _lib
    table = _lib.BINDINGS[HEADER]
    text = _text(os.path.join(ROOT, "include", HEADER))
    syms = sorted(set(re.findall(r"\b(pcnn_[a-z0-9_]+)\s*\(", text)))             # found without the parser
    assert sorted(table) == syms == PINNED
    for s in syms:
        fn = getattr(L, s)                                                         # AttributeError: not exported
        assert fn.restype is table[s][0], s
        assert list(fn.argtypes) == table[s][1], s
        decl = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text).group(1)
        assert len(fn.argtypes) == len(decl.split(",")), s
    assert "PCNN_ABI_VERSION" not in text
    assert re.findall(r"^#include (\S+)$", text, flags=re.M) == ["<stddef.h>", "<stdint.h>"]


def test_header_texts_reads_the_subdirectory():
    from posecnn_amd import _lib
    names = [n for n, _ in _lib.header_texts()]
    top = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    sub = sorted(os.path.relpath(p, os.path.join(ROOT, "include")).replace(os.sep, "/")
                 for p in glob.glob(os.path.join(ROOT, "include", "*", "*.h")))
    assert names == top + sub and sub == [HEADER]
    assert _lib.header_abi_version() == 2


def test_symbols_are_exported_and_have_one_home(L):
    from posecnn_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3 and f[1] in "Tt"}
    assert set(PINNED) <= exported
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        assert not set(re.findall(r"\b(pcnn_[a-z0-9_]+)\s*\(", _text(path))) & set(PINNED), path


def test_header_compiles_alone_as_c11(tmp_path):
    src = tmp_path / "one.c"
    src.write_text('#include "%s"\nint main(void) { return PCNN_POSE_POLISH_LDS_RECORDS == 1024 ? 0 : 1; }\n' % HEADER)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                   check=True)


def test_ops_exports_the_polish():
    from posecnn_amd import ops
    assert "pose_polish" in ops.__all__ and callable(ops.pose_polish)
