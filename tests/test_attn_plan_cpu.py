"""The attention launch selection (csrc/attn_plan.h) against the launches recorded from the host code it was moved out of.

tests/golden/attn_plan.json holds, for 376 calls of ug_attn_fwd and ug_attn_bwd (47 shapes, each with and without the split-head
workspace, RoPE tables and dbias), every launch the earlier host code made: kernel and template arguments, grid, block, the AttnArgs
fields the selection sets, the finishing pass and the stand-alone ug_rope / ug_colsum_bf16 calls.  The test compiles
tests/attn_plan_dump.cpp (attn_plan.h alone, for the host, under ASan + UBSan), feeds it every recorded input and requires the plan
to describe exactly the recorded launches.  How a plan becomes launches (`expected_fwd` / `expected_bwd`) mirrors ug_attn_fwd /
ug_attn_bwd of attention.hip, which the GPU suites run at every kernel.
"""
import json
import os
import shutil
import subprocess

import pytest

import test_attention_edges_gpu as edges

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ml-unigen_amd", "csrc")
HD = 128
FWD = ["attn_fwd32_kernel<4>", "attn_fwd_kernel<8>", "attn_fwd_kernel<4>"]
DQ = ["attn_bwd_dq32_kernel<4>", "attn_bwd_dq_kernel"]
DKV = ["attn_bwd_dkv_dma_kernel", "attn_bwd_dkv_kernel<true>", "attn_bwd_dkv_kernel<false>"]
FINISH = [None, "dkv_finish_rope_kernel", "dkv_finish_kernel"]
FWD_FIELDS = ["kernel", "grid", "block", "order"]
BWD_FIELDS = ["dq", "dq_grid", "dq_order", "dq_fused", "dkv", "dkv_heads", "dkv_grid", "dkv_order", "finish", "rpb", "finish_grid",
              "rope_dq", "colsum_dq", "rope_dk", "colsum_dk", "colsum_dv"]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "attn_plan.json")) as f:
        g = json.load(f)
    return [dict(zip(g["row_columns"], r)) for r in g["rows"]]


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/attn_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "attn_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [[int(v) for v in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def plan_fwd(dumper, shapes):
    return [dict(zip(FWD_FIELDS, p)) for p in dumper(["fwd %d %d %d %d" % tuple(s) for s in shapes])]


def plan_bwd(dumper, problems):
    """problems: (B, L, H, HKV, ws, rope, dbias)"""
    return [dict(zip(BWD_FIELDS, p)) for p in dumper(["bwd %d %d %d %d %d %d %d" % tuple(s) for s in problems])]


def expected_fwd(p):
    """The launch of ug_attn_fwd under plan p, in the golden file's kernel_columns."""
    return [[FWD[p["kernel"]], p["grid"], p["block"], p["order"], 0, 0, 0, 0]]


def expected_bwd(r, p):
    """The launches and stand-alone passes of ug_attn_bwd for problem r under plan p."""
    out = [[DQ[p["dq"]], p["dq_grid"], 256, p["dq_order"], 0, int(p["dq_fused"] and r["rope"]), int(p["dq_fused"] and r["dbias"]), 0]]
    if p["rope_dq"]:
        out.append(["ug_rope", "dq", r["H"]])
    if p["colsum_dq"]:
        out.append(["ug_colsum_bf16", "dq", r["H"] * HD])
    out.append([DKV[p["dkv"]], p["dkv_grid"], 256, p["dkv_order"], p["dkv_heads"], 0, 0, 0])
    if FINISH[p["finish"]] == "dkv_finish_rope_kernel":
        out.append(["dkv_finish_rope_kernel", p["finish_grid"], 256, p["rpb"], r["rope"], r["dbias"]])
    elif FINISH[p["finish"]] == "dkv_finish_kernel":
        out.append(["dkv_finish_kernel", p["finish_grid"], 256])
    if p["rope_dk"]:
        out.append(["ug_rope", "dk", r["HKV"]])
    if p["colsum_dk"]:
        out.append(["ug_colsum_bf16", "dk", r["HKV"] * HD])
    if p["colsum_dv"]:
        out.append(["ug_colsum_bf16", "dv", r["HKV"] * HD])
    return out


def test_every_recorded_attention_launch_is_reproduced(golden, dumper):
    assert len(golden) >= 376
    key = lambda r: (r["B"], r["L"], r["H"], r["HKV"])
    fwd = plan_fwd(dumper, [key(r) for r in golden])
    bwd = plan_bwd(dumper, [key(r) + (r["ws"], r["rope"], r["dbias"]) for r in golden])
    bad = []
    for r, pf, pb in zip(golden, fwd, bwd):
        assert (r["rc_fwd"], r["rc_bwd"]) == (0, 0)
        # a pass a plan asks for has something to do, and the fused stores are only planned with something to fuse
        assert pb["rope_dq"] <= r["rope"] and pb["rope_dk"] <= r["rope"] and max(pb["colsum_dq"], pb["colsum_dk"], pb["colsum_dv"]) <= r["dbias"]
        want = (expected_fwd(pf), expected_bwd(r, pb))
        if want != (r["fwd"], r["bwd"]):
            bad.append((r, want))
    assert not bad, "%d of %d rows differ; first: %r" % (len(bad), len(golden), bad[0])


def test_table_holds_the_suites_and_the_benchmarks_shapes(golden):
    """Every shape the GPU suites and the benchmark run is a row, in all eight combinations of workspace, RoPE tables and dbias."""
    have = {(r["B"], r["L"], r["H"], r["HKV"], r["ws"], r["rope"], r["dbias"]) for r in golden}
    shapes = edges.SHAPES + edges.BIG_SHAPES + [(16, 771, 12, 2), (16, 387, 12, 2), (16, 1603, 12, 2)]
    shapes += [(2, 70, 2, 1), (1, 200, 12, 2), (2, 129, 6, 2), (8, 333, 24, 4), (6, 400, 24, 4), (2, 128, 6, 2), (1, 256, 12, 2), (35, 260, 12, 2),
               (6, 400, 12, 2)]                                       # test_kernels_gpu.py's two attention tests
    for s in shapes:
        for flags in range(8):
            assert tuple(s) + (flags >> 2 & 1, flags >> 1 & 1, flags & 1) in have, s


def test_edge_suite_shapes_select_the_kernels_their_table_names(dumper):
    """tests/test_attention_edges_gpu.py says, per shape, which kernels it is there to run (KERNELS): the plan agrees, and over the
    two lists every kernel and finish the plan can return is run at least once."""
    shapes = edges.SHAPES + edges.BIG_SHAPES
    assert set(edges.KERNELS) == set(shapes) and len(shapes) == len(set(shapes))
    fwd = plan_fwd(dumper, shapes)
    # the call the GPU tests make with RoPE tables and dbias; ops.attn_bwd passes the split-head workspace when H > HKV
    bwd = plan_bwd(dumper, [s + (int(s[2] > s[3]), 1, 1) for s in shapes])
    for s, pf, pb in zip(shapes, fwd, bwd):
        got = dict(fwd=FWD[pf["kernel"]], dq=DQ[pb["dq"]], dkv=DKV[pb["dkv"]], heads=pb["dkv_heads"], finish=FINISH[pb["finish"]])
        assert got == edges.KERNELS[s], s
    # without RoPE tables and dbias the split-head kernels end in the plain finish, whatever HKV
    plain = plan_bwd(dumper, [s + (int(s[2] > s[3]), 0, 0) for s in shapes])
    assert all(FINISH[p["finish"]] == ("dkv_finish_kernel" if s[2] > s[3] else None) for s, p in zip(shapes, plain))
    named = list(edges.KERNELS.values())
    assert {k["fwd"] for k in named} == set(FWD)
    assert {k["dq"] for k in named} == set(DQ)
    assert {k["dkv"] for k in named} == set(DKV)
    assert {k["finish"] for k in named} == set(FINISH)
    assert {k["heads"] for k in named} == {0, 1, 2}
