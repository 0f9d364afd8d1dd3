"""ug_head_score without a GPU: the two symbols are declared, bound and exported; every argument error comes back as -1 with a
message that names it, before any launch; the launch geometry of csrc/head_score_plan.h (compiled alone for the host under ASan +
UBSan, as tests/test_attn_plan_cpu.py does it) covers [0, R) x [0, V) exactly once with column tiles that do not know R and the
workspace bytes the entry point reports; and tests/head_score_ref.py restates torch.log_softmax / argmax."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from head_score_ref import bf16_round64, bf16_steps, head_score_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ml-unigen_amd", "csrc")
RS = [1, 16, 17, 64, 65, 4096]
VS = [1, 255, 256, 257, 4099, 159867]


def test_symbols_are_declared_bound_and_exported():
    from unigen_hip import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unigen_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(lib.LIB_PATH)
    for name, nargs in (("ug_head_score_ws_bytes", 2), ("ug_head_score", 15)):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert len(lib.SIGNATURES[name]) == nargs and hasattr(L, name)
    assert lib.load().ug_abi_version() == lib.ABI_VERSION == 7              # additions do not bump the version


def test_argument_errors_name_the_problem():
    from unigen_hip import lib
    L = lib.load()
    buf = np.zeros(4096, dtype=np.uint8)
    p = (buf.ctypes.data + 15) & ~15                        # a host address stands in: nothing is dereferenced before the checks
    R, V, K = 4, 100, 64

    def call(x=p, ldx=K, R=R, W=p, ldw=K, V=V, K=K, labels=p, ws=p, logp=p):
        rc = L.ug_head_score(x, ldx, R, W, ldw, V, K, labels, -100, ws, logp, None, None, None, None)
        return rc, L.ug_last_error().decode()

    for kw, word in ((dict(K=48, ldx=48, ldw=48), "multiple of 32"), (dict(K=0), "multiple of 32"), (dict(ldx=K - 8), "ldx >= K"),
                     (dict(ldw=K - 8), "ldw >= K"), (dict(logp=None), "logp must not be null"), (dict(ws=None), "ws must not be null"),
                     (dict(labels=None), "labels must not be null"), (dict(x=None), "x and W must not be null"),
                     (dict(R=0), "R >= 1"), (dict(V=0), "V >= 1"), (dict(R=-3), "R >= 1"), (dict(x=p + 2), "16B aligned")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg and msg.startswith("ug_head_score:"), (kw, rc, msg)
    for R_, V_ in ((0, 5), (5, 0), (-1, -1)):
        assert L.ug_head_score_ws_bytes(R_, V_) == -1 and "ug_head_score_ws_bytes" in L.ug_last_error().decode()
    assert L.ug_head_score_ws_bytes(2 ** 24, 2 ** 24) == -1 and "split the rows" in L.ug_last_error().decode()
    with pytest.raises(lib.UniGenHipError):
        from unigen_hip import ops
        ops.head_score(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16), 8, torch.zeros(2, dtype=torch.int64))


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/head_score_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("head_score_plan") / "head_score_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "head_score_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [[int(v) for v in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


FIELDS = ["br", "row_tiles", "col_tiles", "grid", "finish_grid", "label_off", "ws_bytes", "bv", "finish_rows", "part_bytes"]


def test_plan_covers_the_problem_once_and_columns_do_not_know_R(dumper):
    from unigen_hip import lib
    L = lib.load()
    cases = [(R, V) for R in RS for V in VS]
    plans = [dict(zip(FIELDS, p)) for p in dumper(["plan %d %d" % c for c in cases])]
    wgs = dumper(["wgs %d %d" % c for c in cases])
    col_edges = {}
    for (R, V), pl, flat in zip(cases, plans, wgs):
        assert pl["br"] in (32, 64) and pl["bv"] == 256
        pairs = list(zip(flat[0::2], flat[1::2]))
        assert len(pairs) == pl["grid"] == pl["row_tiles"] * pl["col_tiles"] and len(set(pairs)) == len(pairs)      # every tile once
        assert set(pairs) == {(r, c) for r in range(pl["row_tiles"]) for c in range(pl["col_tiles"])}
        rows, cols = np.zeros(R, dtype=np.int64), np.zeros(V, dtype=np.int64)
        for r in range(pl["row_tiles"]):
            assert r * pl["br"] < R                                                        # no empty tile
            rows[r * pl["br"]:min(R, (r + 1) * pl["br"])] += 1
        for c in range(pl["col_tiles"]):
            assert c * pl["bv"] < V
            cols[c * pl["bv"]:min(V, (c + 1) * pl["bv"])] += 1
        assert (rows == 1).all() and (cols == 1).all()
        # the finishing launch reaches every row; the workspace is partials [col_tiles][R] then one fp32 per row, and the library agrees
        assert pl["finish_grid"] * pl["finish_rows"] >= R > (pl["finish_grid"] - 1) * pl["finish_rows"]
        assert pl["label_off"] == pl["col_tiles"] * R * pl["part_bytes"] and pl["label_off"] % 16 == 0
        assert pl["ws_bytes"] == pl["label_off"] + 4 * R == L.ug_head_score_ws_bytes(R, V)
        # O(R x column tiles): nowhere near R x V x 2 bytes once V spans more than a few tiles
        assert pl["ws_bytes"] <= 16 * R * (V // 256 + 1) + 4 * R
        col_edges.setdefault(V, set()).add((pl["col_tiles"], pl["bv"]))
    assert all(len(v) == 1 for v in col_edges.values()), col_edges                         # same column tiles for every R
    assert [dict(zip(FIELDS, p))["br"] for p in dumper(["plan %d 256" % R for R in (1, 32, 33, 64, 65, 130)])] == [32, 32, 64, 64, 64, 64]
    assert dumper(["plan 0 5", "plan 5 0"]) == [[0, 0, 0, 0, 0, 0, 0, 256, 4, 16]] * 2      # no plan for an empty problem


def test_reference_restates_log_softmax_and_argmax():
    g = torch.Generator().manual_seed(11)
    x = torch.randn((7, 96), generator=g).to(torch.bfloat16)
    W = (torch.randn((300, 96), generator=g) * 0.3).to(torch.bfloat16)
    W[40] = W[7]                                             # a tie between two entries: the lower index wins
    x[0] = W[7] * 4
    labels = torch.tensor([3, 299, -100, 0, 300, -1, 150])
    o = head_score_ref(x, W, labels, chunk=128)              # three chunks, the last one ragged
    s = (x.double() @ W.double().t())
    sb = s.to(torch.float32).to(torch.bfloat16).double()     # fp64 -> fp32 is exact enough here not to move a bf16 rounding
    assert torch.equal(bf16_round64(s), sb)
    ls = torch.log_softmax(sb, dim=1)
    ok = torch.tensor([True, True, False, True, False, False, True])
    assert torch.equal(o.valid, ok)
    assert torch.allclose(o.logp[ok], ls[torch.arange(7), labels.clamp(0, 299)][ok], rtol=0, atol=1e-12) and (o.logp[~ok] == 0).all()
    assert torch.allclose(o.lse, torch.logsumexp(sb, dim=1), rtol=0, atol=1e-12)
    assert torch.equal(o.best_logit, sb.max(dim=1).values)
    first = torch.tensor([int((sb[r] == sb[r].max()).nonzero()[0]) for r in range(7)])
    assert torch.equal(o.best, first) and int(o.best[0]) == 7 and sb[0, 40] == sb[0, 7]
    assert torch.equal(o.label_logit[ok], sb[torch.arange(7), labels.clamp(0, 299)][ok])
    # the rounding helpers on known values: 257 is a midpoint between 256 and 258 (ties to even: 256), 259 -> 260
    t = torch.tensor([257.0, 259.0, 1.00390625, -3.0, 0.0, 2.0 ** -20], dtype=torch.float64)
    assert bf16_round64(t).tolist() == [256.0, 260.0, 1.0, -3.0, 0.0, 2.0 ** -20]
    assert bf16_steps(torch.tensor([1.0, 256.0, -1.0, 0.5]), torch.tensor([1.0078125, 258.0, 1.0, 0.5])).tolist()[:2] == [1, 1]
    assert bf16_steps(torch.tensor([0.5]), torch.tensor([0.5])).item() == 0
