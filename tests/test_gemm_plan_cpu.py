"""The bf16 GEMM kernel selection (csrc/gemm_plan.h) against the launches recorded from the host code it was moved out of.

tests/golden/gemm_plan.json holds, for 1102 calls of ug_gemm_bf16 and the three fused entries, every launch the earlier host code
made: kernel and template arguments, grid, block, the GemmArgs fields the selection sets, and the tail_finish launch.  The test
compiles tests/gemm_plan_dump.cpp (gemm_plan.h alone, for the host, under ASan + UBSan), feeds it every recorded input and requires
the plan to describe exactly the recorded launches.  How a plan becomes launches (`expected_gemm` below) mirrors run_plan<> and
launch_p10<> of gemm_bf16.hip, which the GPU suites run at every kernel form.
"""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ml-unigen_amd", "csrc")
BF16, F32, RESID, ROPE, SWIGLU, SWIGLU_BWD = range(6)
K128, K256, K256_SLICED, KP10 = range(4)
# GemmArgs fields the recorded code left unwritten (null) in launches of kernels that do not read them; a plan holds these
NEUTRAL = {"full_tiles": 0, "tail_split": 1, "tail_private": 1, "has_ws": 0}


def up(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "gemm_plan.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dumper(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/gemm_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "gemm_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [[int(v) for v in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def gemm_line(r):
    """r: a gemm row as a dict of the golden file's gemm_columns."""
    return "gemm %d %d %d %d %d %d %d %d %d %d %d %d %d" % (
        r["M"], r["N"], r["K"], r["epi"], r["ak"], r["bk"], r["beta"], r["handle"], r["heights"], r["policy"],
        up(r["N"], 8) + r["ldc_off"], up(r["N"], 8) if r["epi"] == RESID else 0, int(r["bias"] != 2))


PLAN_FIELDS = ["kind", "dbuf", "height", "f0", "f1", "grid_x", "grid_y", "tiles_m", "tiles_n", "full_tiles", "tail_split", "tail_private",
               "uses_workspace", "finish_tiles", "one_barrier", "wide_epilogue"]


def expected_gemm(r, plan):
    """The launches of ug_gemm_bf16 for problem r under `plan`, in the golden file's launch_columns (names, not indices)."""
    p = dict(zip(PLAN_FIELDS, plan))
    args = [p["tiles_m"], p["tiles_n"], p["full_tiles"], p["tail_split"], p["tail_private"], p["uses_workspace"], p["one_barrier"], p["wide_epilogue"]]
    if p["kind"] == K128:
        return [["ug_gemm_bf16", "gemm_kernel", r["epi"], r["ak"], r["bk"], p["dbuf"], p["grid_x"], p["grid_y"], 256] + args + [None]]
    if p["kind"] == KP10:
        return [["ug_gemm_bf16(p10)", "gemm_kernel_p10", r["epi"], r["bk"], p["f0"], p["f1"], p["grid_x"], p["grid_y"], 512] + args + [None]]
    sliced = p["kind"] == K256_SLICED
    out = [["ug_gemm_bf16(p8 k-sliced)" if sliced else "ug_gemm_bf16(p8)", "gemm_kernel_p8", r["epi"], r["ak"], r["bk"], p["one_barrier"],
            p["grid_x"], p["grid_y"], 512] + args + [None]]
    if p["finish_tiles"]:
        out.append(["ug_gemm_bf16(partial sum)" if sliced else "ug_gemm_bf16(tail finish)", "tail_finish_kernel", r["epi"], None, None, None,
                    p["finish_tiles"] * 16, 1, 256] + args + [p["finish_tiles"]])
    return out


def recorded(golden, idx):
    """(rc, launches) of outputs[idx] with names for the site / kernel indices and the unwritten fields made neutral."""
    cols = golden["launch_columns"]
    rc, launches = golden["outputs"][idx][0], []
    for l in golden["outputs"][idx][1:]:
        l = [golden["sites"][l[0]], golden["kernels"][l[1]]] + l[2:]
        if len(l) > 2:
            for name, neutral in NEUTRAL.items():
                i = cols.index(name)
                if l[i] is None:
                    assert l[1] in ("gemm_kernel", "gemm_kernel_p10"), l      # only kernels that never read the field
                    l[i] = neutral
        launches.append(l)
    return rc, launches


def gemm_rows(golden):
    cols = golden["gemm_columns"]
    return [dict(zip(cols, r)) for r in golden["gemm_rows"]]


def test_every_recorded_gemm_launch_is_reproduced(golden, dumper):
    rows = gemm_rows(golden)
    assert len(rows) >= 700
    plans = dumper([gemm_line(r) for r in rows])
    bad = []
    for r, plan in zip(rows, plans):
        rc, launches = recorded(golden, r["out"])
        assert rc == 0
        want = expected_gemm(r, plan)
        if want != launches:
            bad.append((r, want, launches))
    assert not bad, "%d of %d rows differ; first: %r" % (len(bad), len(rows), bad[0])


def test_table_reaches_every_plan_kind_on_the_automatic_path(golden, dumper):
    """Every branch of plan_gemm occurs among the automatic rows, so an edit of the table cannot hollow the row-for-row test out."""
    rows = [r for r in gemm_rows(golden) if r["policy"] == -1 and r["ldc_off"] == 0 and r["bias"] == 0]
    plans = [dict(zip(PLAN_FIELDS, p)) for p in dumper([gemm_line(r) for r in rows])]
    both = list(zip(rows, plans))
    on = [(r, p) for r, p in both if r["heights"] == 1]
    k128 = [p for _, p in both if p["kind"] == K128]
    assert sum(p["dbuf"] for p in k128) >= 2
    assert {1, 4, 5, 12, 32} <= {p["grid_y"] for p in k128 if not p["dbuf"]}
    full = [(r, p) for r, p in both if p["kind"] == K256 and p["finish_tiles"] == 0]
    assert len(full) >= 2 and any((r["M"], r["N"], r["K"]) == (12336, 2048, 1536) for r, _ in full)           # qkv at 12 336 rows
    tails = [(r, p) for r, p in both if p["kind"] == K256 and p["finish_tiles"] > 0]
    assert len(tails) >= 2
    assert any((r["M"], r["N"], r["K"], p["finish_tiles"], p["tail_split"]) == (12336, 1536, 159867, 38, 6) for r, p in tails)   # head dgrad
    sliced = [(r, p) for r, p in both if p["kind"] == K256_SLICED]
    long_k = {(r["M"], p["tail_split"]) for r, p in sliced if r["epi"] == BF16 and r["K"] == 159867}
    assert {(7184, 4), (1542, 6)} <= long_k
    small_f32 = {(r["M"], r["N"], p["tail_split"]) for r, p in sliced if r["epi"] == F32 and r["K"] == 12336}
    assert {(2048, 1536, 5), (1536, 1536, 7)} <= small_f32
    assert all(p["finish_tiles"] == p["tiles_m"] * p["tiles_n"] and p["full_tiles"] == 0 for _, p in sliced)
    p10 = [p for _, p in on if p["kind"] == KP10]
    assert {128, 176, 224, 240, 304} <= {p["height"] for p in p10 if p["grid_x"] <= 256}                       # one round
    assert {272, 288, 304, 320} <= {p["height"] for p in p10 if p["grid_x"] > 256}                             # several rounds
    # without a handle no k-sliced form is planned: those problems fall to the 128x128 kernel
    key = lambda r: tuple(r[c] for c in ("M", "N", "K", "epi", "ak", "bk", "beta", "heights"))
    with_ws = {key(r): p for r, p in both if r["handle"] == 1}
    fell = [p for r, p in both if r["handle"] == 0 and key(r) in with_ws and (with_ws[key(r)]["kind"] == K256_SLICED or with_ws[key(r)]["finish_tiles"] > 0)]
    assert len(fell) >= 2 and all(p["kind"] == K128 and not p["uses_workspace"] for p in fell)
    assert not any(p["kind"] == K256_SLICED or p["finish_tiles"] or p["uses_workspace"] for r, p in both if r["handle"] == 0)


FUSED = {"swiglu": (SWIGLU, 0, "ug_gemm_bf16_swiglu(p10)", "ug_swiglu_fwd"), "rope": (ROPE, 0, "ug_gemm_bf16_qkv_rope", "ug_rope"),
         "swiglu_bwd": (SWIGLU_BWD, 1, "ug_gemm_bf16_swiglu_bwd", None)}


def test_fused_entries_take_the_recorded_heights_and_refusals(golden, dumper):
    rows = [dict(zip(golden["fused_columns"], r)) for r in golden["fused_rows"]]
    assert len(rows) >= 3 * (6 * 14 + 1)
    fused = [r for r in rows if r["K"] % 32 == 0]                  # the shapes the entries' argument checks pass to the fused kernel
    other = [r for r in rows if r["K"] % 32 != 0]
    assert len(other) >= 3 and {r["entry"] for r in other} == set(FUSED)

    def col_tiles(r):
        return (2 * r["W"] if r["entry"] == "swiglu" else r["W"]) // 256
    plans = dumper(["fused %d %d %d %d" % (FUSED[r["entry"]][0], r["M"], col_tiles(r), r["forced"]) for r in fused])
    refused = set()
    for r, (h, f0, f1, tiles_m, grid) in zip(fused, plans):
        epi, bkm, site, _ = FUSED[r["entry"]]
        rc, launches = recorded(golden, r["out"])
        if h < 0:
            assert (rc, launches) == (-1, []), r
            refused.add((r["entry"], r["forced"]))
        else:
            assert rc == 0 and launches == [[site, "gemm_kernel_p10", epi, bkm, f0, f1, grid, 1, 512, tiles_m, col_tiles(r), 0, 1, 1, 0, 0, 1, None]], r
    assert refused == ({(e, h) for e in ("swiglu", "rope") for h in (144, 176, 240, 272, 304)} | {("swiglu_bwd", h) for h in (144, 176, 240, 304)})
    # K % 32 != 0: the projection as an ordinary ug_gemm_bf16 call, then the element-wise pass; swiglu_bwd refuses (its caller owns d(act))
    gemms = [r for r in other if r["entry"] != "swiglu_bwd"]
    as_gemm = [dict(M=r["M"], N=2 * r["W"] if r["entry"] == "swiglu" else r["W"], K=r["K"], epi=BF16, ak=0, bk=0, beta=0, handle=r["handle"],
                    heights=1, policy=-1, ldc_off=0, bias=int(r["entry"] == "rope")) for r in gemms]
    for r, g, plan in zip(gemms, as_gemm, dumper([gemm_line(g) for g in as_gemm])):
        rc, launches = recorded(golden, r["out"])
        assert rc == 0 and launches == expected_gemm(g, plan) + [[FUSED[r["entry"]][3]] * 2], r
    for r in other:
        if r["entry"] == "swiglu_bwd":
            assert recorded(golden, r["out"]) == (-1, []), r
