"""The token rules of prompt-lookup speculative decoding without a GPU: tests/spec_ref.py (plain Python) against transformers'
PromptLookupCandidateGenerator on seeded random sequences, csrc/spec_plan.h (what the kernel applies, compiled alone for the host:
tests/spec_plan_dump.cpp) against spec_ref on the same cases, and the edge cases by hand."""
import os
import random
import shutil
import subprocess

import pytest

import spec_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ml-unigen_amd", "csrc")


def _sequences(count=400, seed=20):
    """(h, G, K): small alphabets (5 .. 20 symbols) so that matches are common; every K in 1 .. 7 and G in 1 .. 4 occurs"""
    rnd = random.Random(seed)
    cases = []
    for c in range(count):
        alphabet = rnd.randint(5, 20)
        n = rnd.choice([1, 2, 3, 4, 5]) if c % 10 == 0 else rnd.randint(6, 80)
        cases.append(([rnd.randrange(alphabet) for _ in range(n)], 1 + c % 4, 1 + (c // 4) % 7))
    return cases


CASES = _sequences()


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tests/spec_plan_dump.cpp"
    exe = str(tmp_path_factory.mktemp("spec_plan") / "spec_plan_dump")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "spec_plan_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        out = [[int(v) for v in l.split()] for l in res.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def _ints(v):
    return " ".join(str(int(x)) for x in v)


def test_draft_rule_is_transformers_prompt_lookup():
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except ImportError:
        pytest.skip("the installed transformers has no PromptLookupCandidateGenerator (generation/candidate_generator.py)")
    import torch
    assert {c[1] for c in CASES} == {1, 2, 3, 4} and {c[2] for c in CASES} == set(range(1, 8))
    matched = 0
    for h, G, K in CASES:
        gen = PromptLookupCandidateGenerator(num_output_tokens=K, max_matching_ngram_size=G, max_length=len(h) + 100)
        ids = torch.tensor([h], dtype=torch.long)
        cand, _ = gen.get_candidates(ids)
        want = cand[0, len(h):].tolist()
        assert spec_ref.draft(h, G, K) == want, (h, G, K)
        matched += bool(want)
    assert matched >= len(CASES) // 2                    # (the alphabets are small enough for the rule to be exercised)


def test_spec_plan_header_agrees_with_the_python_rules(dump):
    rnd = random.Random(5)
    lines, want = [], []
    for h, G, K in CASES:
        lines.append(f"D {G} {K} {len(h)} {_ints(h)}")
        d = spec_ref.draft(h, G, K)
        want.append(d)
    got = dump(lines)
    for (h, G, K), (ngram, start, ln), d in zip(CASES, got, want):
        assert h[start:start + ln] == d and ln == len(d), (h, G, K)
        assert (ngram == 0) == (not d) and ngram <= min(G, len(h) - 1)
        if d:
            assert h[start - ngram:start] == h[len(h) - ngram:]
    # accept and emit on random picks: drafts that agree with the picks for a random number of leading rows, stop ids, widths
    lines, want = [], []
    for _ in range(300):
        nd = rnd.randint(0, 7)
        tok = [rnd.randrange(12) for _ in range(nd + 1)]
        good = rnd.randint(0, nd)
        g = [tok[s + 1] if s < good else rnd.randrange(12) for s in range(nd)] + [rnd.randrange(12)]
        a = spec_ref.accept(g, tok, nd)
        lines.append(f"A {nd} {_ints(g)} {_ints(tok)}")
        want.append([a])
        stops = rnd.sample(range(12), rnd.randint(0, 3))
        emitted, width = rnd.randint(0, 9), rnd.randint(1, 12)
        emitted = min(emitted, width - 1)
        out, done = spec_ref.emit(g, a, stops, emitted, width)
        lines.append(f"E {a} {len(stops)} {_ints(stops)} {emitted} {width} {_ints(g[:a + 1])}".replace("  ", " "))
        want.append([len(out), int(done)])
    assert dump(lines) == want


def test_edge_cases(dump):
    # a history of length 1: nothing can match
    assert spec_ref.draft([3], 4, 7) == [] and dump(["D 4 7 1 3"]) == [[0, 0, 0]]
    # a match whose continuation runs into the end: the draft stops at the end of the history
    h = [1, 2, 9, 9, 1, 2]
    assert spec_ref.draft(h, 2, 7) == [9, 9, 1, 2] and dump([f"D 2 7 6 {_ints(h)}"]) == [[2, 2, 4]]
    assert spec_ref.draft([5, 6, 7, 5], 1, 2) == [6, 7] and spec_ref.draft([5, 6, 7, 5], 1, 7) == [6, 7, 5]
    # only the suffix matches itself: no earlier occurrence, no draft; a shorter n-gram may still match
    assert spec_ref.draft([1, 2, 3, 4], 2, 5) == [] and dump(["D 2 5 4 1 2 3 4"]) == [[0, 0, 0]]
    assert spec_ref.draft([4, 2, 3, 4], 2, 5) == [2, 3, 4] and dump(["D 2 5 4 4 2 3 4"]) == [[1, 1, 3]]
    # the earliest match wins, and the longest n-gram that has one
    assert spec_ref.draft([1, 2, 7, 1, 2, 8, 1, 2], 2, 1) == [7]
    assert spec_ref.draft([3, 2, 7, 1, 2, 8, 1, 2], 2, 1) == [8] and spec_ref.draft([2, 7, 1, 2, 8, 9, 2], 2, 1) == [7]
    # a stop id inside an accepted run: emitted up to and including it, done, the rest of the run dropped
    g, tok = [4, 5, 6, 7], [9, 4, 5, 6]
    assert spec_ref.accept(g, tok, 3) == 3
    assert spec_ref.emit(g, 3, [5], 0, 100) == ([4, 5], True)
    assert dump(["A 3 4 5 6 7 9 4 5 6", "E 3 1 5 0 100 4 5 6 7"]) == [[3], [2, 1]]
    # a cut at width: done without a stop id; exactly reaching the width is done too
    assert spec_ref.emit(g, 3, [], 8, 10) == ([4, 5], True) and spec_ref.emit(g, 3, [], 6, 10) == ([4, 5, 6, 7], True)
    assert spec_ref.emit(g, 3, [], 5, 10) == ([4, 5, 6, 7], False)
    assert dump(["E 3 0 8 10 4 5 6 7", "E 3 0 6 10 4 5 6 7", "E 3 0 5 10 4 5 6 7"]) == [[2, 1], [4, 1], [4, 0]]
    # a first draft token that is wrong: only the model's own pick is emitted
    assert spec_ref.accept([1, 5, 6, 7], tok, 3) == 0 and spec_ref.emit([1, 5, 6, 7], 0, [], 0, 10) == ([1], False)
    # the state machine: first token (no advance), then a step that accepts two of three drafted tokens
    ref = spec_ref.SpecRef([7, 8, 9, 1, 7], S=4, G=2, K=3, width=10, pos=20)
    assert ref.verify([8], [0, 0, 0, 0], advance=False) == [8, 9, 1, 7] and (ref.pos, ref.steps, ref.n_draft) == (20, 0, 3)
    assert ref.verify([9, 1, 2, 5], ref.tok) == [2, 2, 2, 2]
    assert (ref.out, ref.pos, ref.steps, ref.drafted, ref.accepted, ref.n_draft) == ([8, 9, 1, 2], 23, 1, 3, 2, 0)
