"""Host tier of the workspace layouts: every ``*_workspace_bytes`` function against the committed size table, the bump arena
itself (a stand-alone C++ program), and the one refusal of a short or null workspace (no device is touched before it)."""
import ctypes
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "workspace_sizes.json")
TOOL = os.path.join(ROOT, "tools", "workspace_sizes.py")
P = 256                    # placeholder pointer: non-null, 256-byte aligned, never dereferenced


def _lib_or_skip(names=()):
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in tuple(names) + ("nrl_last_error",):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def test_every_workspace_size_matches_the_committed_table():
    """tools/workspace_sizes.py on the built library, with no NRL_* switch set, reproduces tests/data/workspace_sizes.json byte for
    byte.  A pull request that changes a layout on purpose regenerates the file with the tool."""
    from newsreclib_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NRL_")}
    out = subprocess.run([sys.executable, TOOL, _lib.LIB_PATH], capture_output=True, text=True, check=True, env=env, cwd=ROOT).stdout
    want_text = open(TABLE).read()
    got, want = json.loads(out), json.loads(want_text)
    exported = sorted(n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes"))
    assert sorted(want) == exported == sorted(got)
    for name in exported:
        for g, w in zip(got[name], want[name]):
            assert g == w, (name, g, w)
        assert len(got[name]) == len(want[name]) >= 4, name
    assert out == want_text


def test_arena_check_program(tmp_path):
    """tests/arena_check.cpp includes only nrl_arena.h: a few hundred pseudo-random take sequences, measured and carved."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "arena_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "newsreclib_amd", "csrc"),
                    os.path.join(ROOT, "tests", "arena_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "arena_check OK: 400 sequences" in run.stdout


def test_arena_header_needs_no_hip():
    text = open(os.path.join(ROOT, "newsreclib_amd", "csrc", "nrl_arena.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and all(inc in ("<stddef.h>", "<stdint.h>") for inc in includes), includes


def _caum_score_bwd(lib, ws, ws_bytes):
    B, C, H, N2, U = 3, 5, 50, 100, 400
    return lib.nrl_caum_score_bwd(P, P, P, P, P, P, P, P, B, C, 0, H, N2, U, P, P, P, P, P, ws, ws_bytes, None)


def _miner_poly_bwd(lib, ws, ws_bytes):
    B, max_hist, D, Cd, K = 3, 50, 400, 200, 32
    return lib.nrl_miner_poly_bwd(P, P, P, P, P, P, B, max_hist, D, Cd, K, P, P, P, P, ws, ws_bytes, None)


def _dkn_click_bwd(lib, ws, ws_bytes):
    from newsreclib_amd import _lib
    p = _lib.NrlDknClickParams(P, P, P, P, P, P, P, P, 16)
    g = _lib.NrlDknClickGrads(P, P, P, P, P, P, P, P)
    B, max_hist, max_cand, dim = 3, 50, 5, 400
    return lib.nrl_dkn_click_bwd(ctypes.byref(p), ctypes.byref(g), P, P, max_hist, P, P, B, max_cand, dim, P, P, P, P, ws, ws_bytes, None)


@pytest.mark.parametrize("entry,size_fn,size_args,call", [
    ("nrl_caum_score_bwd", "nrl_caum_score_workspace_bytes", (3, 5, 50, 100), _caum_score_bwd),
    ("nrl_miner_poly_bwd", "nrl_miner_poly_workspace_bytes", (3, 32, 200), _miner_poly_bwd),
    ("nrl_dkn_click_bwd", "nrl_dkn_click_workspace_bytes", (3, 5, 400, 16), _dkn_click_bwd),
])
def test_short_and_null_workspaces_are_refused_before_any_launch(entry, size_fn, size_args, call):
    """One byte short: NRL_E_WORKSPACE (-2) and the shared message; null: NRL_E_INVALID (-1).  Every pointer is a placeholder that
    is never read, so both returns happen before the entry touches the device."""
    lib = _lib_or_skip((entry, size_fn))
    need = getattr(lib, size_fn)(*size_args)
    assert need > 256
    assert call(lib, P, need - 1) == -2
    msg = lib.nrl_last_error().decode()
    assert "workspace too small: %d < %d bytes" % (need - 1, need) in msg, msg
    assert call(lib, None, need) == -1
    assert "workspace" in lib.nrl_last_error().decode()
    assert call(lib, P + 16, need) == -1                   # misaligned
