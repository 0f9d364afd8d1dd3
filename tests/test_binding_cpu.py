"""The ctypes binding is derived from include/unigen_hip.h (unigen_hip/lib.py: parse_header); none of this needs a GPU: the
parser on synthetic text, the derived table against the recorded ABI v7 one, the two call surfaces against the built library,
the bench tags against recorded strings, and the import of lib.py without torch."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYNTHETIC = """
/* a header in the style of unigen_hip.h
 * int ug_fake(int x);   <- inside a comment: not a prototype */
#ifndef T_H
#define T_H
#include <stdint.h>
extern "C" {
#define UG_ABI_VERSION 42
typedef struct ug_handle ug_handle;
const char* ug_last_error(void);
int ug_create(ug_handle** out);
#define UG_SOME_FLAG 0x100   /* between two prototypes */
int64_t ug_bytes(const ug_handle* h);          // a value, not a status
int ug_many(int n, const void* const* p, const int64_t *ld,
            float* const* dw /* [n] or null */, int64_t rows, float eps,
            hipStream_t stream);
}
#endif
"""


def test_parser_on_synthetic_header_text():
    from unigen_hip import lib
    P, I64, I32, F32 = lib.P, lib.I64, lib.I32, lib.F32
    protos, version = lib.parse_header(SYNTHETIC)
    assert version == 42
    assert list(protos) == ["ug_last_error", "ug_create", "ug_bytes", "ug_many"]          # the header's order; ug_fake is a comment
    assert protos["ug_last_error"] == (ctypes.c_char_p, [], [], [])
    assert protos["ug_create"] == (ctypes.c_int, [P], ["out"], ["ug_handle**"])
    assert protos["ug_bytes"] == (ctypes.c_int64, [P], ["h"], ["const ug_handle*"])
    many = protos["ug_many"]
    assert many.restype is ctypes.c_int
    assert many.names == ["n", "p", "ld", "dw", "rows", "eps", "stream"]
    assert many.c_types == ["int", "const void* const*", "const int64_t*", "float* const*", "int64_t", "float", "hipStream_t"]
    want = [I32, P, P, P, I64, F32, P]
    assert len(many.argtypes) == len(want) and all(a is b for a, b in zip(many.argtypes, want))
    assert lib.parse_header("int ug_x(void);")[1] is None                                  # no version defined
    # nothing is guessed: every other type fails, naming the prototype
    for bad in ("int ug_bad(const float* x, double scale, hipStream_t stream);", "int ug_bad(unsigned n);", "int ug_bad(size_t n);",
                "int ug_bad(float v[4]);", "int ug_bad(int (*cb)(int));", "int ug_bad(int);", "double ug_bad(int n);",
                "void ug_bad(int n);"):
        with pytest.raises(lib.UniGenHipError, match="ug_bad"):
            lib.parse_header(bad)


def test_abi_v7_is_frozen():
    """tests/golden/abi_v7.json was recorded from the last hand-written table, before the binding was derived: that revision's
    lib.py loaded by file path, every SIGNATURES entry written as its list of kinds with the return kind its load() set (I64 for
    ug_comm_bytes_on_wire, I32 otherwise), plus ug_last_error (no arguments, a C string), which load() bound outside the table.
    112 entries, then the same set of names as the header's.  Every recorded prototype must be derived unchanged; names the
    record does not have are later additions and are allowed."""
    from unigen_hip import lib
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_v7.json")))
    assert len(golden) == 112
    kinds = {"P": lib.P, "I64": lib.I64, "I32": lib.I32, "F32": lib.F32}
    returns = {"I32": ctypes.c_int, "I64": ctypes.c_int64, "STR": ctypes.c_char_p}
    assert lib.ABI_VERSION >= 7
    for name, rec in golden.items():
        assert name in lib.PROTOTYPES, name
        proto = lib.PROTOTYPES[name]
        assert proto.restype is returns[rec["ret"]], name
        assert len(proto.argtypes) == len(rec["args"]) and all(a is kinds[k] for a, k in zip(proto.argtypes, rec["args"])), name
        if name != "ug_last_error":
            assert lib.SIGNATURES[name] is proto.argtypes
    assert "ug_last_error" not in lib.SIGNATURES and set(lib.SIGNATURES) | {"ug_last_error"} == set(lib.PROTOTYPES)


def test_call_surfaces_against_the_built_library():
    from unigen_hip import lib
    so = ctypes.CDLL(lib.LIB_PATH)
    missing = [name for name in lib.PROTOTYPES if not hasattr(so, name)]
    assert not missing, missing
    raw, api = lib.load(), lib.api()
    assert api is lib.api()
    assert set(vars(api)) == set(lib.PROTOTYPES) and lib.VALUE_RETURNS <= set(lib.PROTOTYPES)
    bad_gemm = (0, 0, 80, 0, 0, 80, 0, 0, 8, 16, 16, 68, 0, 0, 0, 0, 0, 0, -1, 0)          # K % 8 != 0, both row-major: rejected before any launch
    assert raw.ug_gemm_bf16(*bad_gemm) == -1                                              # the raw surface returns the status
    message = raw.ug_last_error()
    assert b"multiple of 8" in message
    with pytest.raises(lib.UniGenHipError) as via_check:
        lib.check(-1, "ug_gemm_bf16")                                                     # the message is still the thread's last one
    with pytest.raises(lib.UniGenHipError) as via_api:
        api.ug_gemm_bf16(*bad_gemm)
    assert raw.ug_last_error() == message
    assert str(via_api.value) == str(via_check.value) == "ug_gemm_bf16 failed (rc=-1): " + message.decode()
    assert api.ug_decode_sw_supported(0, 0, 0, 0) == 0                                    # a value: handed back, not checked
    assert api.ug_gemm_set_fused_tile_height(0) is None                                   # a status of 0: nothing to say
    assert api.ug_abi_version() == lib.ABI_VERSION


def test_profile_tags_are_built_from_parameter_names(monkeypatch):
    """The expected strings were recorded from the last positional form of `_profiled` (args[9], args[10], ...) on these very
    argument lists."""
    from unigen_hip import lib

    class Recorder:
        def __init__(self):
            self.on = []

        def record(self, stream):
            self.on.append(stream)

    monkeypatch.setattr(lib, "_event_pair", lambda sp: (Recorder(), Recorder(), ("stream", sp)))
    LA = ctypes.c_int64 * 2
    cases = [
        ("ug_gemm_bf16", (0, 11, 80, 1, 12, 96, 0, 13, 64, 384, 256, 1536, 2, 0, 0, 0, 1, 0, -1, 5),
         "gemm", "ug_gemm_bf16[M=384 N=256 K=1536 ak=1 bk=0 epi=2]"),
        ("ug_conv3x3_split", (1, 2, 3, 4, 0, 5, 2, 16, 24, 32, 128, 128, 77, 0, 0, 0, 0, 6, 32, 5),
         "tokenizer_and_towers", "ug_conv3x3_split[B=2 16x24 32->128 gn=1]"),
        ("ug_conv3x3_split", (1, 2, 3, 4, 0, 5, 2, 16, 24, 32, 128, 128, 0, 0, 0, 0, 0, 6, 32, 5),
         "tokenizer_and_towers", "ug_conv3x3_split[B=2 16x24 32->128 gn=0]"),
        ("ug_gemm_bf16_wgrad_group", (2, None, None, None, None, None, None, LA(256, 512), LA(1536, 8960), None, LA(64, 12336), 5),
         "gemm", "ug_gemm_bf16_wgrad_group[256x1536x64 512x8960x12336]"),
        ("ug_rope", (0,) * 9 + (5,), "elementwise", "ug_rope"),
    ]
    for name, args, family, tag in cases:
        assert len(args) == len(lib.SIGNATURES[name])
        seen = []

        def stub(*a):
            seen.append(a)
            return 0 if len(seen) < 3 else -2
        raw, checked = lib._profiled(name, stub, lib.PROTOTYPES[name].names, lambda: b"stub message")
        monkeypatch.setattr(lib, "PROFILE", None)
        assert raw(*args) == 0 and seen == [args]                                         # off: the call and nothing else
        prof = {}
        monkeypatch.setattr(lib, "PROFILE", prof)
        assert checked(*args) is None
        (e0, e1, got), = prof[family]
        assert got == tag and e0.on == e1.on == [("stream", 5)]                            # bracketed on the stream passed last
        with pytest.raises(lib.UniGenHipError, match=rf"^{name} failed \(rc=-2\): stub message$"):
            checked(*args)
        assert [t for _, _, t in prof[family]] == [tag, tag] and list(prof) == [family]
    # a tag field the header does not declare fails when the wrapper is made, not at the first profiled call
    with pytest.raises(lib.UniGenHipError, match="a_kmajor"):
        lib._profiled("ug_gemm_bf16", stub, ["h", "A", "M", "N", "K", "b_kmajor", "epilogue", "stream"], lambda: b"")


def test_lib_imports_by_file_path_without_torch():
    child = ("import importlib.util, sys\n"
             "spec = importlib.util.spec_from_file_location('ug_lib_sigs', sys.argv[1])\n"
             "m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)\n"
             "assert 'torch' not in sys.modules, 'lib.py imported torch'\n"
             "assert m.SIGNATURES and m.ABI_VERSION >= 7 and m.HEADER_PATH.endswith('unigen_hip.h')\n"
             "print(len(m.SIGNATURES))\n")
    res = subprocess.run([sys.executable, "-c", child, os.path.join(ROOT, "ml-unigen_amd", "unigen_hip", "lib.py")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert int(res.stdout) >= 111
