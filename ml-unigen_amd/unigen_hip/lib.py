"""ctypes binding of libunigen_hip.so (the C ABI declared in include/unigen_hip.h).

The header is the table: every prototype in it is parsed at import and the ctypes argument and return types are derived from
it, so the binding cannot drift from the declarations the compiler checks every definition against.  tests/test_binding_cpu.py
freezes the derived ABI v7 table against a recorded one and tests/test_host_cpu.py checks the library's exports against it.

The product path has no CPU fallback: if the shared library is missing the import of any op fails
loudly with the build command.  Nothing under oracle/ is ever imported from here.
"""
import collections
import ctypes
import os
import re
import subprocess
import types

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
LIB_PATH = os.environ.get("UNIGEN_HIP_LIB") or os.path.join(CSRC_DIR, "libunigen_hip.so")     # (probe builds: tools/probes/_build/*.so)
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "unigen_hip.h"))

P = ctypes.c_void_p
I64 = ctypes.c_int64
I32 = ctypes.c_int
F32 = ctypes.c_float


class UniGenHipError(RuntimeError):
    pass


# ---- the header's prototypes -> ctypes.  Nothing is guessed: a type outside these two maps fails the import, naming the prototype.
_SCALARS = {"int64_t": I64, "int": I32, "float": F32, "hipStream_t": P}
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
# restype / argtypes: ctypes types; names / c_types: the header's parameter names and their C spellings
Proto = collections.namedtuple("Proto", "restype argtypes names c_types")


def _c_type(text):
    return re.sub(r"\*(?=\w)", "* ", re.sub(r"\s*\*\s*", "*", text.strip()))      # one spelling: `const void* const*`


def parse_header(text):
    """C header text -> ({name: Proto} for every `RET ug_name(params);` in the header's order, UG_ABI_VERSION or None)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+UG_ABI_VERSION[ \t]+(\d+)[ \t]*$", text, re.M)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    protos = {}
    for stmt in re.split(r"[;{}]", text):
        if "(" not in stmt:
            continue                                   # typedefs, `extern "C"`
        stmt = " ".join(stmt.split())
        m = re.fullmatch(r"([\w \*]+?) ?\b(ug_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            raise UniGenHipError(f"unigen_hip.h: cannot bind `{stmt}`: not of the form RET ug_name(TYPE name, ...)")
        ret, name, params = _c_type(m.group(1)), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise UniGenHipError(f"unigen_hip.h: {name}: no ctypes mapping for the return type `{ret}`")
        argtypes, names, c_types = [], [], []
        for param in ([] if params == "void" else params.split(",")):
            pm = re.fullmatch(r"(.*[\w\*]) ?\b(\w+)", param.strip())
            c = _c_type(pm.group(1)) if pm else ""
            if "*" in c:
                kind = P
            elif c in _SCALARS:
                kind = _SCALARS[c]
            else:
                raise UniGenHipError(f"unigen_hip.h: {name}: no ctypes mapping for the parameter `{param.strip()}`")
            argtypes.append(kind)
            names.append(pm.group(2))
            c_types.append(c)
        protos[name] = Proto(_RETURNS[ret], argtypes, names, c_types)
    return protos, (int(version.group(1)) if version else None)


with open(HEADER_PATH) as _f:
    PROTOTYPES, ABI_VERSION = parse_header(_f.read())
if ABI_VERSION is None:
    raise UniGenHipError(f"{HEADER_PATH} defines no UG_ABI_VERSION")
SIGNATURES = {name: proto.argtypes for name, proto in PROTOTYPES.items() if name != "ug_last_error"}    # name -> argtypes
# entry points whose return value is a value, not a status: api() hands it back unchecked
VALUE_RETURNS = frozenset(("ug_abi_version", "ug_decode_sw_supported", "ug_text_sample_workspace_ints", "ug_head_score_ws_bytes",
                           "ug_comm_bytes_on_wire", "ug_beam_candidates_ws_bytes"))

_lib = None
_api = None

# Launch-time breakdown by kernel family (bench.py's `roofline_by_family`): when PROFILE is a dict, every entry point that
# launches on the caller's stream is bracketed by a pair of HIP events recorded on torch's current stream -- the stream every
# op passes down (or the explicit stream of an overlapped launch, e.g. the optimizer update) -- and filed under its family.  None (the default) costs one global read per call.
PROFILE = None


def family_of(name):
    if name.startswith("ug_gemm_bf16"):
        return "gemm"
    if name in ("ug_attn_fwd", "ug_attn_bwd", "ug_attn_prefill_cached"):
        return "attention"
    if name.startswith(("ug_conv", "ug_groupnorm", "ug_amax", "ug_lfq", "ug_nchw", "ug_nhwc", "ug_gemm_f32", "ug_softmax_rows", "ug_linear_",
                        "ug_layernorm", "ug_siglip")):
        return "tokenizer_and_towers"
    if name in ("ug_adamw_flat", "ug_adamw_flat_dev"):
        return "adamw"
    if name in ("ug_attn_decode_seq", "ug_spec_verify"):
        return "spec_decode"                    # the two launches a speculative verify step adds to the decode forms' own
    return "elementwise"


# bench tags that carry the launch's shape: entry point -> (the header's parameter names, format of their values)
_TAGS = {
    "ug_gemm_bf16": (("M", "N", "K", "a_kmajor", "b_kmajor", "epilogue"),
                     lambda *v: "ug_gemm_bf16[M=%d N=%d K=%d ak=%d bk=%d epi=%d]" % v),
    "ug_conv3x3_split": (("B", "H", "W", "Cin", "Cout", "gn_mu_rstd"),
                         lambda *v: "ug_conv3x3_split[B=%d %dx%d %d->%d gn=%d]" % (v[:5] + (1 if v[5] else 0,))),
    "ug_gemm_bf16_wgrad_group": (("n", "rows", "cols", "K"),
                                 lambda n, rows, cols, K: "ug_gemm_bf16_wgrad_group[%s]" % " ".join("%dx%dx%d" % (rows[i], cols[i], K[i]) for i in range(n))),
}


def _tagger(name, names):
    """args -> the bench tag of one call; the tag's fields are resolved to argument positions here, once"""
    if name not in _TAGS:
        return lambda args: name
    fields, fmt = _TAGS[name]
    missing = [f for f in fields if f not in names]
    if missing:
        raise UniGenHipError(f"{name}: its profile tag reads the parameters {missing}, which include/unigen_hip.h does not declare")
    idx = [names.index(f) for f in fields]
    return lambda args: fmt(*[args[i] for i in idx])


def _event_pair(sp):
    """two timing events and the torch stream that the raw hipStream_t `sp` is"""
    import torch
    sp = getattr(sp, "value", sp) or 0
    cur = torch.cuda.current_stream()
    st = cur if sp == cur.cuda_stream else torch.cuda.ExternalStream(sp)
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), st


def _failure(name, rc, last_error):
    return UniGenHipError(f"{name} failed (rc={rc}): {last_error().decode('utf-8', 'replace')}")


def _profiled(name, fn, names, last_error):
    """(raw, checked) forms of a launching entry point: both time the launch when PROFILE is set; `raw` returns the status,
    `checked` raises UniGenHipError on a non-zero one"""
    fam, tag_of = family_of(name), _tagger(name, names)

    def timed(prof, args):
        e0, e1, st = _event_pair(args[-1])             # every launching entry point takes its stream last
        e0.record(st)
        rc = fn(*args)
        e1.record(st)
        prof.setdefault(fam, []).append((e0, e1, tag_of(args)))
        return rc

    def raw(*args):
        prof = PROFILE
        return fn(*args) if prof is None else timed(prof, args)

    def checked(*args):
        prof = PROFILE
        rc = fn(*args) if prof is None else timed(prof, args)
        if rc != 0:
            raise _failure(name, rc, last_error)
    raw.__name__ = checked.__name__ = name
    return raw, checked


def _checked(name, fn, last_error):
    def checked(*args):
        rc = fn(*args)
        if rc != 0:
            raise _failure(name, rc, last_error)
    checked.__name__ = name
    return checked


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise UniGenHipError("building libunigen_hip.so failed (see output above)")
    return LIB_PATH


def load():
    """The library with every entry point bound to the header's prototype; its functions return the raw status."""
    global _lib, _api
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise UniGenHipError(
            f"{LIB_PATH} is missing: the HIP extension is the only implementation of this path "
            f"(no CPU fallback). Build it with `make -C {CSRC_DIR}` or `python -c 'import __graft_entry__ as g; g.build()'`.")
    # torch ships its own libamdhip64.so.7; whichever copy of that soname is mapped first serves the whole process.
    # Loading ours first maps /opt/rocm's runtime, and a later `import torch` then runs on a HIP/HSA mix that finds no
    # device -- so torch's runtime always goes first (the host side of this library is PyTorch anyway).
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    checked = types.SimpleNamespace()
    last_error = lib.ug_last_error
    for name, proto in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes, fn.restype = proto.argtypes, proto.restype
        if name in VALUE_RETURNS or name == "ug_last_error":
            setattr(checked, name, fn)
        elif proto.c_types[-1:] != ["hipStream_t"] or name.startswith("ug_comm_"):      # launches nothing / runs on its own streams
            setattr(checked, name, _checked(name, fn, last_error))
        else:
            raw, chk = _profiled(name, fn, proto.names, last_error)
            setattr(lib, name, raw)
            setattr(checked, name, chk)
    if lib.ug_abi_version() != ABI_VERSION:
        raise UniGenHipError(f"ABI version mismatch: library reports {lib.ug_abi_version()}, binding expects {ABI_VERSION}")
    _lib, _api = lib, checked
    return lib


def api():
    """The checked call surface: api().ug_x(*args) launches and raises UniGenHipError itself on a non-zero status (the
    VALUE_RETURNS entries hand their value back as it is)."""
    if _api is None:
        load()
    return _api


def check(rc, name="ug call"):
    if rc != 0:
        raise _failure(name, rc, load().ug_last_error)
