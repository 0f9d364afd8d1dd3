"""ug_maskgit_step_ex (include/unigen_hip.h) without a GPU: the symbol is declared, exported and bound, the ABI version did not move,
and the argument checks answer before any memory is touched.  Plain ctypes calls on host buffers."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ug_maskgit_step_ex"


def _bufs(N, n, V, ld):
    """host memory of the right sizes for one cfg call (never dereferenced: without a GPU the launch itself fails)"""
    rows = N * n
    return {
        "logits": (ctypes.c_uint16 * (2 * rows * ld))(),
        "u_sample": (ctypes.c_float * rows)(), "u_conf": (ctypes.c_float * rows)(),
        "cur": (ctypes.c_int64 * rows)(), "sampled": (ctypes.c_int64 * rows)(), "sel": (ctypes.c_float * rows)(),
        "next_cur": (ctypes.c_int64 * rows)(), "next_ids": (ctypes.c_int64 * rows)(),
        "logp": (ctypes.c_float * (2 * rows))(), "stats": (ctypes.c_float * (2 * rows))(),
    }


def _call(L, b, N, n, V, ld, sample_temperature=1.0, top_k=0, top_p=1.0, min_p=0.0):
    a = {k: ctypes.addressof(v) for k, v in b.items()}
    return L.ug_maskgit_step_ex(a["logits"], ld, V, N, n, 1, 2.0, a["u_sample"], a["u_conf"], a["cur"], 7, 0, 3, 0.6, sample_temperature,
                                top_k, top_p, min_p, a["sampled"], a["sel"], a["next_cur"], a["next_ids"], 0, a["logp"], a["stats"], 0)


def test_maskgit_step_ex_is_declared_exported_and_bound():
    from unigen_hip import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unigen_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, text)
    assert hasattr(ctypes.CDLL(lib.LIB_PATH), NAME)
    assert NAME in lib.SIGNATURES and len(lib.SIGNATURES[NAME]) == 26
    assert lib.SIGNATURES[NAME][:14] == lib.SIGNATURES["ug_maskgit_step"][:14]        # ug_maskgit_step's arguments come first, in order
    assert lib.load().ug_abi_version() == lib.ABI_VERSION == 7


def test_maskgit_step_ex_all_zero_call_is_an_argument_error():
    from unigen_hip import lib
    L = lib.load()
    rc = L.ug_maskgit_step_ex(*([0] * 26))
    assert rc == -1 and b"ug_maskgit_step_ex" in L.ug_last_error()


def test_maskgit_step_ex_refuses_bad_filters_and_a_row_too_long_for_lds():
    from unigen_hip import lib
    L = lib.load()
    N, n = 1, 4
    b = _bufs(N, n, 8193, 8200)
    assert _call(L, b, N, n, 8193, 8200, top_k=5) == -1 and b"8192" in L.ug_last_error()
    assert _call(L, b, N, n, 8193, 8200, sample_temperature=0.8) == -1 and b"8192" in L.ug_last_error()
    b = _bufs(N, n, 64, 64)
    for kw in ({"top_p": 0.0}, {"top_p": 1.5}, {"min_p": -0.1}, {"min_p": 1.5}, {"top_k": -1}, {"sample_temperature": 0.0}):
        assert _call(L, b, N, n, 64, 64, **kw) == -1 and b"bad filter" in L.ug_last_error(), kw
    assert _call(L, b, N, n, 64, 63) == -1 and b"bad sizes" in L.ug_last_error()          # ld < V


def test_maskgit_step_ex_well_formed_call_reaches_the_launch():
    """without a GPU a well-formed call fails at the launch (-2), like ug_maskgit_step: every argument check passed"""
    import torch
    from unigen_hip import lib
    if torch.cuda.is_available():
        return                                                    # (on a GPU the launch would run on host pointers)
    L = lib.load()
    N, n, V = 1, 4, 64
    b = _bufs(N, n, V, V)
    a = {k: ctypes.addressof(v) for k, v in b.items()}
    want = L.ug_maskgit_step(a["logits"], V, V, N, n, 1, 2.0, a["u_sample"], a["u_conf"], a["cur"], 7, 0, 3, 0.6, a["sampled"], a["sel"],
                             a["next_cur"], a["next_ids"], 0, 0)
    assert want == -2
    assert _call(L, b, N, n, V, V) == -2 and b"launch failed" in L.ug_last_error()                         # the parent's kernel + outputs
    assert _call(L, b, N, n, V, V, sample_temperature=0.8, top_k=5, top_p=0.9, min_p=0.01) == -2           # the filtered kernel
