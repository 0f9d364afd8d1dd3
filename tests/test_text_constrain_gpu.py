"""ug_text_constrain + ug_text_stop_seq (csrc/text_sampler.hip) through ops.text_constrain_ / ops.text_stop_seq_: exact, against
text_constraints_ref.py.

Constrain, the grid: every pair of V in {77, 4 099, 159 867 (the real vocabulary)} and R in {1, 3, 32}; both row layouts (ld = V rounded
up to 8, and ld = V, the deterministic head's); n in {0, 1, 2, 4} x step in {2, 3, 6} against min_new = 3 (below, at, above); the
prompt-history lengths {0, 5, 37} rotating over the rows.  Logits as test_text_penalize_gpu.py builds them: 3 x randn (not
bf16-representable), distinct patterns behind V and in a guard row, with 0.0, -0.0 and +inf planted at biased ids.  Bias ids
include 0 and V - 1; three ids are suppressed.  Histories and tokens draw from four ids so that n-grams repeat; the columns of the token
buffer at and behind the step, and the history entries behind a row's length, hold the same kind of ids and must not count.
Planted cases: a history of one repeated id, an n-gram that straddles the prompt / emitted boundary, a history shorter than n - 1, ids
outside [0, V) in the history.
Stop sequences: lengths {2, 3, 16}, ns in {1, 8}; a match at the earliest possible step, only a proper suffix matching, two sequences
matching in one step, a row already done, the last unfinished row (steps_used), and m > step + 1 against a guard column."""
import pytest
import torch

import repetition_penalty_ref as pref
import text_constraints_ref as ref

pytestmark = pytest.mark.gpu

NINF = float("-inf")
NSTEPS, LDH, MIN_NEW = 8, 40, 3


def _logits(V, R, ld, seed):
    g = torch.Generator().manual_seed(seed + 1)
    full = torch.empty(R + 1, ld)
    full[:, :V] = 3.0 * torch.randn(R + 1, V, generator=g)
    full[:, V:] = 1e30 + 1e24 * torch.arange(ld - V)[None]        # distinct patterns behind V
    full[R] = 7e29 + 1e24 * torch.arange(ld)                        # the guard row
    return full


def _bias(V):
    """(id, bias): ids 0 and V - 1, a bias that is no bf16 value, three suppressed ids"""
    return [(0, 1.5), (V - 1, -0.7001), (10, 2.0 ** -9), (11, -3.25), (12, 0.5), (13, 100.0), (14, -1e-3), (20, NINF), (V - 2, NINF), (5, NINF)]


def _case(V, R, seed):
    g = torch.Generator().manual_seed(seed)
    hist = torch.randint(0, 4, (R, LDH), generator=g, dtype=torch.int32)
    toks = torch.randint(0, 4, (R, NSTEPS), generator=g, dtype=torch.int32)
    return hist, toks


def _state(dev, R, step):
    from unigen_hip import ops
    st = ops.text_state(R, dev)
    st[0:1].fill_(step)
    return st


@pytest.mark.parametrize("R", [1, 3, 32])
@pytest.mark.parametrize("V", [77, 4099, 159867])
def test_constrain_is_exact_on_the_grid(dev, V, R):
    from unigen_hip import ops
    hist, toks = _case(V, R, seed=V + R)
    bias = _bias(V)
    stop = [V - 3, 1, 13]
    pairs, stop_d = ops.text_bias_pairs(bias, dev), torch.tensor(stop, dtype=torch.long, device=dev)
    assert tuple(pairs.shape) == (len(bias), 2) and pairs.dtype == torch.int32
    hist_d, toks_d = hist.to(dev), toks.to(dev)
    for ld in (ops.round_up(V, 8), V):
        full = _logits(V, R, ld, seed=V + R)
        for r in range(R):
            full[r, 0], full[r, 12], full[r, 10] = -2.7, -0.0, 0.0
            if r % 3 == 1:
                full[r, 13], full[r, 20] = float("inf"), float("inf")
        full_d = full.to(dev)
        for k, (n, step) in enumerate((n, step) for n in (0, 1, 2, 4) for step in (2, 3, 6)):
            lens = torch.tensor([(0, 5, 37)[(r + k) % 3] for r in range(R)], dtype=torch.int32)
            want = full.clone().numpy()
            for r in range(R):
                ref.device_rule(want[r], V, bias, MIN_NEW, stop, n, hist[r, :int(lens[r])].tolist(), toks[r].tolist(), step)
            want = torch.from_numpy(want)
            assert not pref.same_bits(want, full) and pref.same_bits(want[R], full[R]) and pref.same_bits(want[:, V:], full[:, V:])
            got = []
            for _ in range(2):                                      # twice on the same inputs: a function of them
                lg = full_d.clone()
                state = _state(dev, R, step)
                ops.text_constrain_(lg[:R], V, state, toks_d, bias=pairs, min_new=MIN_NEW, stop_ids=stop_d, ngram=n, hist=hist_d, hist_len=lens.to(dev))
                assert state.tolist() == _state(dev, R, step).tolist()                       # the state block is read, never written
                got.append(lg.cpu())
            assert pref.same_bits(got[0], got[1])
            bad = int((got[0].view(torch.int32) != want.view(torch.int32)).sum())
            assert bad == 0, (ld, n, step, bad)
    assert torch.equal(toks_d.cpu(), toks) and torch.equal(hist_d.cpu(), hist)


def _run(dev, V, R, full, n, step, hist_rows, toks_rows, bias=None, min_new=0, stop=None):
    """one launch on planted histories (lists per row) -> the logits back on the CPU, [R + 1, ld] with the guard row"""
    from unigen_hip import ops
    hist = torch.full((R, LDH), 1, dtype=torch.int32)
    lens = torch.zeros(R, dtype=torch.int32)
    toks = torch.full((R, NSTEPS), 1, dtype=torch.int32)
    for r in range(R):
        lens[r] = len(hist_rows[r])
        hist[r, :len(hist_rows[r])] = torch.tensor(hist_rows[r], dtype=torch.int64).to(torch.int32)
        toks[r, :len(toks_rows[r])] = torch.tensor(toks_rows[r], dtype=torch.int32)
    lg = full.to(dev)
    ops.text_constrain_(lg[:R], V, _state(dev, R, step), toks.to(dev), bias=None if bias is None else ops.text_bias_pairs(bias, dev), min_new=min_new,
                        stop_ids=None if stop is None else torch.tensor(stop, dtype=torch.long, device=dev), ngram=n,
                        hist=hist.to(dev) if any(hist_rows) else None, hist_len=lens.to(dev) if any(hist_rows) else None)
    want = full.clone().numpy()
    for r in range(R):
        ref.device_rule(want[r], V, bias or [], min_new, stop or [], n, [int(e) for e in hist[r, :int(lens[r])].tolist()], toks[r].tolist(), step)
    got = lg.cpu()
    assert pref.same_bits(got, torch.from_numpy(want))
    return got


def _banned(got, full, r):
    """the entries of row r that changed, all of which must now hold -inf"""
    changed = (got[r].view(torch.int32) != full[r].view(torch.int32)).nonzero().flatten().tolist()
    assert all(float(got[r, e]) == NINF for e in changed)
    return changed


def test_constrain_planted_histories(dev):
    V, R = 77, 4
    full = _logits(V, R, 80, seed=9)
    # (a) one repeated id: every n bans it (and only it) once the history holds n - 1 of them
    got = _run(dev, V, R, full, 2, 0, [[7] * 10, [7], [], [7] * 3], [[]] * R)
    assert [_banned(got, full, r) for r in range(R)] == [[7], [], [], [7]]
    got = _run(dev, V, R, full, 4, 2, [[7] * 10, [7], [], [7] * 2], [[7, 7]] * R)
    assert [_banned(got, full, r) for r in range(R)] == [[7], [], [], [7]]          # (row 1: T = 3 = n - 1, no earlier 4-gram; row 2: T = 2)
    # (b) the 3-gram 5 6 9 starts in the prompt history and ends in the emitted tokens; the suffix 5 6 is emitted
    got = _run(dev, V, R, full, 3, 4, [[2, 5, 6], [5], [], [2, 5, 6]], [[9, 1, 5, 6], [6, 9, 5, 6], [5, 6, 9, 5], [9, 1, 5, 3]])
    assert [_banned(got, full, r) for r in range(R)] == [[9], [9], [], []]
    # the same tokens one step earlier: the last emitted column does not count yet
    got = _run(dev, V, R, full, 3, 3, [[2, 5, 6], [5], [], [2, 5, 6]], [[9, 1, 5, 6], [6, 9, 5, 6], [5, 6, 9, 5], [9, 1, 5, 3]])
    assert [_banned(got, full, r) for r in range(R)] == [[], [], [], []]
    # (c) a history shorter than n - 1 changes nothing at all
    got = _run(dev, V, R, full, 4, 1, [[3], [], [], [3]], [[3], [3], [3], [3]])
    assert pref.same_bits(got, full)
    # (d) ids outside [0, V) behind a matching prefix are never used as an index; inside a prefix they compare as numbers
    big = 2 ** 31 - 1
    got = _run(dev, V, R, full, 2, 0, [[3, V + 5, 3, -1, 3, 8, 3, big, 3], [3, V, 3], [-7, 4, -7], [3, -2 ** 31, 3]], [[]] * R)
    assert [_banned(got, full, r) for r in range(R)] == [[8], [], [4], []]
    got = _run(dev, V, R, full, 3, 2, [[V, 3, 5, 0], [big, 3, V], [], []], [[V, 3], [big, 3], [V, 3], [1, 1]])
    assert [_banned(got, full, r) for r in range(R)] == [[5], [], [], []]
    # n = 1 bans every id of the history that is an index; min_new alone holds the stop ids back only below the bound
    got = _run(dev, V, R, full, 1, 2, [[0, V - 1, V, -1], [], [4], []], [[6, 7, 50]] * R)
    assert [_banned(got, full, r) for r in range(R)] == [[0, 6, 7, V - 1], [6, 7], [4, 6, 7], [6, 7]]
    got = _run(dev, V, R, full, 0, 2, [[]] * R, [[]] * R, min_new=3, stop=[V - 1, 0, V, -5])
    assert [_banned(got, full, r) for r in range(R)] == [[0, V - 1]] * R
    got = _run(dev, V, R, full, 0, 3, [[]] * R, [[]] * R, min_new=3, stop=[V - 1, 0])
    assert pref.same_bits(got, full)


def test_constrain_refuses_bad_arguments(dev):
    from unigen_hip import ops
    from unigen_hip.lib import UniGenHipError
    V, R = 100, 2
    lg = torch.zeros(R, V, device=dev)
    toks = torch.zeros((R, NSTEPS), dtype=torch.int32, device=dev)
    state = ops.text_state(R, dev)
    with pytest.raises(UniGenHipError, match="bad constraints"):
        ops.text_constrain_(lg, V, state, toks, ngram=17)
    with pytest.raises(UniGenHipError, match="bad constraints"):
        ops.text_constrain_(lg, V, state, toks, bias=ops.text_bias_pairs([(e, 1.0) for e in range(1025)], dev))
    with pytest.raises(UniGenHipError, match="bad sizes"):
        ops.text_constrain_(lg, V + 1, state, toks, ngram=2)
    with pytest.raises(UniGenHipError):
        ops.text_constrain_(lg, V, state, toks.long(), ngram=2)
    with pytest.raises(UniGenHipError):
        ops.text_constrain_(lg, V, state, toks, ngram=2, hist=torch.zeros((R, 4), dtype=torch.int32, device=dev))
    with pytest.raises(UniGenHipError):
        ops.text_stop_seq_(*ops.text_stop_seqs([[1] * 17], dev), toks, state)
    with pytest.raises(UniGenHipError):
        ops.text_stop_seq_(*ops.text_stop_seqs([[1, 2]] * 9, dev), toks, state)
    assert not bool(lg.any()) and state.tolist()[:3] == [0, R, 0]


# ------------------------------------------------------------------ stop sequences
A, B, C = (30, 31), (29, 30, 31), tuple(range(40, 56))
EIGHT = [(1, 2), A, (3, 4, 5), B, C, (60, 61), (62, 63, 64), (65, 66)]
W = 24


def _stop_case(dev, seqs, rows, step, done, guard=None):
    """rows: per row the emitted tokens [0 .. step]; the buffer behind `step` holds 31s (a tail that must not count); guard: the row in
    front of row 0 in memory.  -> (state, lengths) from the device, after checking them against the restatement"""
    from unigen_hip import ops
    R = len(rows)
    big = torch.full((R + 1, W), 31, dtype=torch.int32)
    if guard is not None:
        big[0] = torch.tensor(guard, dtype=torch.int32)
    for r, row in enumerate(rows):
        assert len(row) == step + 1
        big[1 + r, :step + 1] = torch.tensor(row, dtype=torch.int32)
    state = [step + 1, R - sum(done), 0, 0] + list(done) + [0] * (32 - R)
    lengths = [W] * R
    big_d = big.to(dev)
    state_d = torch.tensor(state, dtype=torch.int32, device=dev)
    len_d = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ids, off = ops.text_stop_seqs(seqs, dev)
    assert off.tolist()[-1] == ids.numel() == sum(len(s) for s in seqs)
    ops.text_stop_seq_(ids, off, big_d[1:], state_d, lengths=len_d)
    ref.stop_seq_step(state, big[1:].tolist(), lengths, seqs, R)
    assert state_d.tolist() == state and len_d.tolist() == lengths and torch.equal(big_d.cpu(), big)
    ops.text_stop_seq_(ids, off, big_d[1:], state_d, lengths=len_d)                   # once more on the result: nobody finishes twice
    assert state_d.tolist() == state and len_d.tolist() == lengths
    state2 = torch.tensor([step + 1, R - sum(done), 0, 0] + list(done) + [0] * (32 - R), dtype=torch.int32, device=dev)
    ops.text_stop_seq_(ids, off, big_d[1:], state2)                                   # lengths may be null
    assert state2.tolist() == state
    return state, lengths


@pytest.mark.parametrize("ns", [1, 8])
def test_stop_sequences_finish_the_right_rows_once(dev, ns):
    step = 15                                                      # the earliest step at which the 16-id sequence can match
    fill = list(range(100, 116))
    rows = [fill[:14] + list(A),                                   # 0: the 2-id sequence
            list(C),                                               # 1: the 16-id sequence, from column 0
            fill[:13] + [9, 30, 31] if ns == 1 else fill[:13] + [9, 4, 5],      # 2: with ns = 8 only the proper suffix 4 5 of 3 4 5
            fill[:13] + list(B),                                   # 3: A and B both complete here
            fill[:14] + list(A),                                   # 4: already done
            fill]                                                  # 5: nothing
    done = [0, 0, 0, 0, 1, 0]
    if ns == 8:
        state, lengths = _stop_case(dev, EIGHT, rows, step, done)
        assert state[4:10] == [1, 1, 0, 1, 1, 0] and state[1] == 2 and state[2] == 0
        assert lengths == [16, 16, W, 16, W, W]
    else:
        for seq, want_done, left in ((A, [1, 0, 1, 1, 1, 0], 2), (B, [0, 0, 0, 1, 1, 0], 4), (C, [0, 1, 0, 0, 1, 0], 4)):
            state, lengths = _stop_case(dev, [seq], rows, step, done)
            assert state[4:10] == want_done and state[1] == left and state[2] == 0
            assert lengths == [16 if d and not w else W for d, w in zip(want_done, done)]


def test_stop_sequence_of_the_last_unfinished_row_sets_steps_used(dev):
    rows = [[7, 8, 9, 30, 31], [7, 8, 9, 30, 31], [1, 2, 3, 4, 5]]
    state, lengths = _stop_case(dev, [A, (3, 4, 5)], rows, 4, [1, 0, 1])
    assert state[:4] == [5, 0, 5, 0] and state[4:7] == [1, 1, 1] and lengths == [W, 5, W]
    state, lengths = _stop_case(dev, [A, (3, 4, 5)], rows, 4, [0, 0, 1])               # two rows finish in one launch
    assert state[:4] == [5, 0, 5, 0] and lengths == [5, 5, W]
    state, lengths = _stop_case(dev, [A], [[30, 31]], 1, [0])                          # m == step + 1 exactly
    assert state[:3] == [2, 0, 2] and lengths == [2]


def test_stop_sequence_longer_than_the_emitted_tokens_never_reads_in_front_of_column_zero(dev):
    """m = 3 > step + 1 = 2: the two emitted tokens are the sequence's last two and the entry in front of column 0 -- the previous row's
    last column, the guard row's for row 0 -- holds its first"""
    guard = [0] * (W - 1) + [29]
    rows = [[30, 31], [30, 31], [30, 29]]
    from unigen_hip import ops
    R, step = 3, 1
    big = torch.full((R + 1, W), 29, dtype=torch.int32)             # every row's tail holds 29 too
    big[0] = torch.tensor(guard, dtype=torch.int32)
    for r, row in enumerate(rows):
        big[1 + r, :2] = torch.tensor(row, dtype=torch.int32)
    state = [step + 1, R, 0, 0] + [0] * 32
    state_d = torch.tensor(state, dtype=torch.int32, device=dev)
    len_d = torch.full((R,), W, dtype=torch.int32, device=dev)
    ids, off = ops.text_stop_seqs([B, C], dev)
    ops.text_stop_seq_(ids, off, big.to(dev)[1:], state_d, lengths=len_d)
    lengths = [W] * R
    ref.stop_seq_step(state, big[1:].tolist(), lengths, [B, C], R)
    assert state_d.tolist() == state == [2, R, 0, 0] + [0] * 32 and len_d.tolist() == [W] * R
    state_d[0:1].fill_(0)                                           # before any pick: step = -1, nothing happens
    ops.text_stop_seq_(ids, off, big.to(dev)[1:], state_d, lengths=len_d)
    assert state_d.tolist() == [0, R, 0, 0] + [0] * 32
