"""tests/elementwise_ref.py without a GPU: the distance constants behind the bars are what an fp32 evaluation on this CPU measures
(within a factor of two), the exactness conditions of the integer-valued RMSNorm backward inputs hold (every intermediate is an fp32
number), the fp32 AdamW restatement is torch.optim.AdamW, and the bars BITE: with the restatement's own fp32 evaluation standing in
for the kernel every bar of tests/test_elementwise_gpu.py passes, and each listed subtly wrong reference is rejected by at least 2 x
on at least one case (docs/experiments.md, "Element-wise kernels: exact and per-element tests", has the table)."""
import functools

import pytest
import torch

import elementwise_ref as ew

BF = torch.bfloat16


def _worst(table, key, d, case):
    if d > table.get(key, (0.0, None))[0]:
        table[key] = (d, case)


# ================================================================================================ the constants
def _measure_rms(t):
    for cols in ew.RMS_FWD_WIDTHS:
        for rows in ew.RMS_FWD_ROWS:
            w, xs = ew.rms_fwd_inputs(rows, cols)
            for x in xs:
                ref = ew.rms_fwd_restated(x, w)
                r, y = ew.rms_fwd_fp32(x, w)
                _worst(t, "RMS_RSTD_DIST", ew.dist(r, ref.rstd, ref.rstd.abs()), (rows, cols))
                _worst(t, "RMS_Y_DIST", ew.dist(y, ref.y, ref.y.abs()), (rows, cols))
                # the restatement's own fp32 evaluation passes every forward bar, bf16 rounding included
                assert ew.rms_rstd_excess(r, ref) <= 1 and ew.rms_y_excess(y, ref) <= 1 and ew.rms_y_excess(y.to(BF), ref) <= 1
    for rows, cols in ew.RMS_BWD_REAL_CASES:
        p = ew.rms_bwd_real_input(rows, cols)
        ref = ew.rms_bwd_restated(p)
        dres, dw = ew.rms_bwd_fp32(p)
        _worst(t, "RMS_BWD_DRES_DIST", ew.dist(dres, ref.dres, ref.dres_a), (rows, cols))
        _worst(t, "RMS_BWD_DW_DIST", ew.dist(dw, ref.dw, ref.dw_a), (rows, cols))


def _adam_steps(name, n):
    """-> per step: (constants fp32, constants float64, state before, gradient, fp32 restatement after)"""
    hp = ew.ADAM_SETS[name]
    p, m, v, grads = ew.adam_state(n, name)
    out = []
    for s, g in enumerate(grads):
        step = hp["first_step"] + s
        c32, c64 = ew.adam_consts(hp, step), ew.adam_consts(hp, step, f64=True)
        after = ew.adam_step(p, g, m, v, c32)[:3]
        out.append((c32, c64, (p, m, v), g, after))
        p, m, v = after
    return out


def _measure_adam(t):
    for name in ew.ADAM_SETS:
        for n in ew.ADAM_SIZES:
            for c32, c64, (p, m, v), g, (p1, m1, v1) in _adam_steps(name, n):
                pd, md, vd, a = ew.adam_step(p.double(), g.double(), m.double(), v.double(), c64)
                _worst(t, "ADAM_P_DIST", ew.dist(p1, pd, a.p), (name, n))
                _worst(t, "ADAM_M_DIST", ew.dist(m1, md, a.m), (name, n))
                _worst(t, "ADAM_V_DIST", ew.dist(v1, vd, a.v), (name, n))


def _measure_gn(t):
    for case in ew.GN_CASES:
        x, ga, be = ew.gn_input(case)
        G = case[4]
        st = ew.gn_stats_restated(x, G)
        assert ew.gn_mean_is_clear_of_ties(st), case
        m32, r32, _ = ew.gn_stats_one_pass(x, G)
        _worst(t, "GN_STAT_DIST", max(ew.dist(m32, st.mean, st.a_mean), ew.dist(r32, st.rstd, st.a_rstd)), case)
        for sw, key in ((False, "GN_Y_DIST"), (True, "GN_SWISH_DIST")):
            v, a = ew.gn_apply_restated(x, ga, be, G, st, sw)
            _worst(t, key, ew.dist(ew.gn_apply_fp32(x, ga, be, G, m32, r32, sw), v, a), case)


def _measure_softmax(t):
    for case in ew.SOFTMAX_CASES:
        for sc in ew.SOFTMAX_SCALES:
            x = ew.softmax_input(case)
            v, a = ew.softmax_restated(x, sc)
            _worst(t, "SOFTMAX_DIST", ew.dist(ew.softmax_fp32(x, sc), v, a), (case, sc))
    x = ew.softmax_input(ew.SOFTMAX_EXTREME, extreme=True)
    v, a = ew.softmax_restated(x, 1.0)
    got = ew.softmax_fp32(x, 1.0)
    assert (got == 0).any() and (v > 0).all(), "exp(-600) is 0 in fp32 and positive in float64"
    assert ew.softmax_excess(got, v, a) <= 1, "the floor is what lets an underflowed element pass -- and only that"
    assert ew.fp32_excess(got, v, a, ew.SOFTMAX_SLACK).max().item() > 1


@functools.lru_cache(maxsize=None)
def _measured():
    t = {}
    for f in (_measure_rms, _measure_adam, _measure_gn, _measure_softmax):
        f(t)
    return t


@pytest.mark.parametrize("name", ["RMS_RSTD_DIST", "RMS_Y_DIST", "RMS_BWD_DRES_DIST", "RMS_BWD_DW_DIST", "ADAM_P_DIST", "ADAM_M_DIST",
                                  "ADAM_V_DIST", "GN_STAT_DIST", "GN_Y_DIST", "GN_SWISH_DIST", "SOFTMAX_DIST"])
def test_constants_are_what_this_cpu_measures(name):
    """each constant within a factor of two of the distance measured here (another CPU's vector maths may differ in the last bits);
    the slack is MARGIN = 4 times the constant"""
    d, case = _measured()[name]
    const = getattr(ew, name)
    print(f"{name}: constant {const:.3g}, measured {d:.3g} at {case}")
    assert const / 2 <= d <= const * 2, (name, const, d, case)
    assert getattr(ew, name.replace("_DIST", "_SLACK")) == ew.MARGIN * const and ew.MARGIN == 4.0
    assert d >= 2.0 ** -25, "an fp32 evaluation is at least half an fp32 rounding from float64 somewhere"


# ================================================================================================ RMSNorm forward: the bars bite
def test_rmsnorm_forward_bars_reject_wrong_references():
    w, (x,) = ew.rms_fwd_inputs(9, 252)
    ref = ew.rms_fwd_restated(x, w)
    # rstd without eps: only the row with |x| ~ 1e-4 shows it (the all-zero row is left alone here: it would be infinite)
    wrong = ew.rms_fwd_restated(x, w, no_eps=True)
    per_row = ew.fp32_excess(wrong.rstd.float(), ref.rstd, ref.rstd.abs(), ew.RMS_RSTD_SLACK)
    assert per_row[2] >= 2 and (per_row[[0, 1, 3, 4, 5, 6, 7, 8]] <= 1).all(), per_row
    assert ew.rms_y_excess(wrong.y.float().to(BF), ref) >= 2
    # the mean over the width rounded up to 256
    wrong = ew.rms_fwd_restated(x, w, pad_to=256)
    assert ew.rms_rstd_excess(wrong.rstd.float(), ref) >= 2 and ew.rms_y_excess(wrong.y.float().to(BF), ref) >= 2
    assert ew.rms_y_excess(wrong.y.float(), ref) >= 2
    # ... which a width that is a multiple of 256 cannot show
    w2, (x2,) = ew.rms_fwd_inputs(9, 256)
    assert ew.rms_rstd_excess(ew.rms_fwd_restated(x2, w2, pad_to=256).rstd.float(), ew.rms_fwd_restated(x2, w2)) <= 1


def test_one_element_four_bf16_ulps_off_fails_the_rule_and_passes_the_old_gate():
    """the gate of test_rmsnorm_fwd_bwd (max-abs <= 0.04 and relative Frobenius error < 4e-3) accepts a y with one element four bf16
    ulps off; the per-element rule rejects it"""
    w, (x,) = ew.rms_fwd_inputs(9, 1536)
    ref = ew.rms_fwd_restated(x, w)
    y = ref.y.float().to(BF)
    assert ew.rms_y_excess(y, ref) <= 1
    r, c = ((ref.y.abs() >= 0.5) & (ref.y.abs() < 0.99)).nonzero()[0].tolist()
    bad = y.clone()
    bad.view(torch.int16)[r, c] += 4                       # sign-magnitude: four ulps up in magnitude
    assert ew.rms_y_excess(bad, ref) >= 2
    old_ref = ref.y.float()                                 # what rmsnorm_ref returns: fp32
    maxabs = (bad.float() - old_ref.to(BF).float()).abs().max().item()
    rel = ((bad.float() - old_ref).norm() / old_ref.norm()).item()
    assert maxabs <= 0.04 and rel < 4e-3, (maxabs, rel)


# ================================================================================================ RMSNorm backward
def _is_fp32(t):
    return torch.equal(t.float().double(), t)


@pytest.mark.parametrize("cols", ew.RMS_BWD_DW_WIDTHS)
@pytest.mark.parametrize("rows", ew.RMS_BWD_ROWS)
def test_integer_rmsnorm_backward_is_exact_in_fp32(rows, cols):
    _check_int_case(rows, cols)


def test_integer_rmsnorm_backward_is_exact_in_fp32_many_rows():
    _check_int_case(*ew.RMS_BWD_MANY_ROWS)


def _check_int_case(rows, cols):
    """dw: every term dy * xhat is a multiple of 0.5 and the sum of their magnitudes (with dw0) stays below 2^23, so every partial sum
    in any order is an fp32 number.  dres at a power-of-two width: every intermediate of the float64 evaluation is an fp32 number, so
    an fp32 evaluation in any order (fused multiply-adds included: an exact product rounds nowhere) gives the same bits.  Summation
    orders are scrambled to show it."""
    p = ew.rms_bwd_int_input(rows, cols)
    ref = ew.rms_bwd_restated(p)
    s = ref.steps
    assert torch.equal(s["dyx"] * 2, (s["dyx"] * 2).round()) and (s["dyx"].abs().sum(0) + p.dw0.abs()).max().item() < 2 ** 23
    assert _is_fp32(ref.dw) and (p.dw0 != 0).all()
    perm = torch.randperm(rows, generator=ew._gen(rows + cols))
    acc = p.dw0.clone()
    for r in perm.tolist():                                # one row at a time, fp32, scrambled
        acc += p.dy[r].float() * (p.x[r] * p.rstd[r])
    assert torch.equal(acc.double(), ref.dw)
    if cols in ew.RMS_BWD_DRES_EXACT_WIDTHS or (rows, cols) == ew.RMS_BWD_MANY_ROWS:
        assert torch.equal(s["gx"] * 4, (s["gx"] * 4).round()) and s["gx"].abs().sum(-1).max().item() < 2 ** 22
        for name, t in s.items():
            assert _is_fp32(t), name
        cperm = torch.randperm(cols, generator=ew._gen(rows * cols))
        xhat, g = p.x * p.rstd[:, None], p.dy.float() * p.w
        dot = (g * xhat)[:, cperm].cumsum(-1)[:, -1:] / cols                       # sequential fp32 sum in a scrambled order
        assert torch.equal((p.dres0 + p.rstd[:, None] * (g - xhat * dot)).double(), ref.dres)
        assert torch.equal(ew.rms_bwd_fp32(p)[0].double(), ref.dres)
    else:
        assert not all(_is_fp32(t) for t in s.values()), "this width is not expected to be exact: dot = sum / cols rounds"


def test_rmsnorm_backward_bars_reject_wrong_references():
    # per-element rule on real inputs
    for rows, cols in ew.RMS_BWD_REAL_CASES:
        p = ew.rms_bwd_real_input(rows, cols)
        ref = ew.rms_bwd_restated(p)
        dres, dw = ew.rms_bwd_fp32(p)
        assert ew.fp32_excess(dres, ref.dres, ref.dres_a, ew.RMS_BWD_DRES_SLACK).max().item() <= 1
        assert ew.fp32_excess(dw, ref.dw, ref.dw_a, ew.RMS_BWD_DW_SLACK).max().item() <= 1
        wrong = ew.rms_bwd_restated(p, pad_to=256)             # dot divided by the padded width
        e = ew.fp32_excess(wrong.dres.float(), ref.dres, ref.dres_a, ew.RMS_BWD_DRES_SLACK).max().item()
        assert e >= 2 if cols % 256 else e <= 1                # (1536 is its own padded width)
        wrong = ew.rms_bwd_restated(p, skip_row_col=(rows - 1, cols - 3))
        assert ew.fp32_excess(wrong.dw.float(), ref.dw, ref.dw_a, ew.RMS_BWD_DW_SLACK).max().item() >= 2
        wrong = ew.rms_bwd_restated(p, stale_quad=(rows - 1, cols - 4))
        assert ew.fp32_excess(wrong.dres.float(), ref.dres, ref.dres_a, ew.RMS_BWD_DRES_SLACK).max().item() >= 2
    # the exact comparisons on integer inputs: any of them is a failed torch.equal
    p = ew.rms_bwd_int_input(17, 252)
    ref = ew.rms_bwd_restated(p)
    assert not torch.equal(ew.rms_bwd_restated(p, skip_row_col=(16, 5)).dw, ref.dw) or p.dy[16, 5] == 0 or p.x[16, 5] == 0
    assert not torch.equal(ew.rms_bwd_restated(p, pad_to=256).dres, ref.dres)
    assert not torch.equal(ew.rms_bwd_restated(p, stale_quad=(16, 248)).dres, ref.dres)
    rows_hit = [(r, c) for r in range(17) for c in range(252) if p.dy[r, c] != 0 and p.x[r, c] != 0]
    assert len(rows_hit) > 0.5 * 17 * 252, "most (row, column) pairs carry a non-zero term: a dropped one shows"


# ================================================================================================ AdamW
def test_fp32_adamw_restatement_is_torch_adamw():
    """from a zero state, the base hyper-parameters: torch.optim.AdamW's single-tensor update within a few fp32 roundings"""
    n, hp = 4099, ew.ADAM_SETS["base"]
    g0 = ew._gen(4)
    p0 = torch.randn(n, generator=g0)
    pr = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pr], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"])
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for step in (1, 2, 3):
        g = torch.randn(n, generator=g0)
        pr.grad = g.clone()
        opt.step()
        p, m, v, _ = ew.adam_step(p, g, m, v, ew.adam_consts(hp, step))
        assert (p - pr.detach()).abs().max().item() < 1e-6
    st = opt.state[pr]
    assert (m - st["exp_avg"]).abs().max().item() < 5e-7 and ((v - st["exp_avg_sq"]).abs() <= 2e-5 * v).all()
    # (v: torch forms 1 - beta2 in double and rounds it, the kernel subtracts in fp32: 1.3e-5 apart, see the next test)


def test_fp32_adamw_restatement_uses_correctly_rounded_operations():
    """sqrt: the IEEE root (numpy's) is the float64 root rounded once, and torch.sqrt is not always it -- why the restatement does
    not use it; the division and the products by a Python scalar are the IEEE operations (numpy's, element by element)"""
    import numpy as np
    _, _, v, grads = ew.adam_state(15367, "base")
    x = v + 1e-3 * grads[0] * grads[0]
    want = torch.sqrt(x.double()).float()
    assert torch.equal(ew.ieee_sqrt(x), want)
    print("torch.sqrt differs from the correctly rounded root in", int((torch.sqrt(x) != want).sum()), "of", x.numel())
    c = ew.adam_consts(ew.ADAM_SETS["base"], 2)
    f = np.float32
    assert torch.equal(x / c.bc2_sqrt, torch.from_numpy(x.numpy() / f(c.bc2_sqrt)))
    assert torch.equal(grads[1] / x, torch.from_numpy(grads[1].numpy() / x.numpy()))
    assert torch.equal(c.step_size * x, torch.from_numpy(f(c.step_size) * x.numpy()))
    assert torch.equal(x * c.beta2 + (c.w2 * grads[1]) * grads[1], torch.from_numpy(x.numpy() * f(c.beta2) + (f(c.w2) * grads[1].numpy()) * grads[1].numpy()))


def test_adamw_float64_reference_needs_the_fp32_rounded_hyper_parameters():
    """1 - float32(0.999) against 1 - 0.999 moves v by more than 1e-5 relative -- over ten times the bar"""
    hp = ew.ADAM_SETS["base"]
    assert abs(ew.adam_consts(hp, 1, f64=True).w2 / (1 - 0.999) - 1) > 1e-5 > 10 * ew.ADAM_V_SLACK


def test_adamw_bars_reject_wrong_references():
    """with the fp32 restatement in the kernel's place the float64 rule passes; a wrong update of each kind fails it by 2 x (and would
    fail the bit-for-bit comparison with the fp32 restatement all the more)"""
    def worst(name, variant, n=4099):
        out = [0.0, 0.0, 0.0]
        for c32, c64, (p, m, v), g, _ in _adam_steps(name, n):
            got = ew.adam_step(p, g, m, v, c32, variant)[:3]
            pd, md, vd, a = ew.adam_step(p.double(), g.double(), m.double(), v.double(), c64)
            for i, (gt, vv, aa, sl) in enumerate(zip(got, (pd, md, vd), (a.p, a.m, a.v), (ew.ADAM_P_SLACK, ew.ADAM_M_SLACK, ew.ADAM_V_SLACK))):
                out[i] = max(out[i], ew.fp32_excess(gt, vv, aa, sl).max().item())
        return out
    for name in ew.ADAM_SETS:
        assert max(worst(name, None)) <= 1, name
    assert worst("base", "decay_after")[0] >= 2                      # decay applied after the update instead of before
    assert worst("base", "eps_inside")[0] >= 2 and worst("large_eps", "eps_inside")[0] >= 2
    w = worst("grad_scale", "scale_m_only")                          # grad_scale applied to m but not to v
    assert w[2] >= 2 and w[0] >= 2 and w[1] <= 1
    # the bias correction of step - 1: steps 2 and 3 of the base set evaluated with the constants of steps 1 and 2
    hp = ew.ADAM_SETS["base"]
    steps = _adam_steps("base", 4099)
    for s in (1, 2):
        c32, c64, (p, m, v), g, _ = steps[s]
        got = ew.adam_step(p, g, m, v, ew.adam_consts(hp, hp["first_step"] + s - 1))[0]
        pd, _, _, a = ew.adam_step(p.double(), g.double(), m.double(), v.double(), c64)
        assert ew.fp32_excess(got, pd, a.p, ew.ADAM_P_SLACK).max().item() >= 2
    # ... which the late steps cannot show (both corrections are 1 to fp32 there): the reason the early steps stay in the list
    hp = ew.ADAM_SETS["late_steps"]
    assert vars(ew.adam_consts(hp, 100000)) == vars(ew.adam_consts(hp, 100001))


# ================================================================================================ cast
def test_cast_expectation_rounds_to_nearest_even_and_truncation_is_rejected():
    sp = ew.cast_input(5)
    want, nan = ew.cast_expected(sp)
    assert [w & 0xffff for w in want.tolist()] == [0x3f80, 0x3f82, 0x7f80, 0x8000, 0x0001] and not nan.any()
    x = ew.cast_pattern()
    want, nan = ew.cast_expected(x)
    assert x.numel() == 5 * 65536 and int(nan.sum()) == 2 * (4 + 127 * 5)      # exponent 255: 0x7f80 with a low half, 0x7f81 .. 0x7fff
    assert ew.is_bf16_nan(want[nan]).all() and not ew.is_bf16_nan(want[~nan]).any()
    trunc = ew.cast_truncated(x)
    differ = (trunc != want) & ~nan
    assert differ.float().mean().item() > 0.3                         # low halves 0x8001 and 0xffff always round up, 0x8000 on odd
    assert torch.equal(trunc[:65536][~nan[:65536]], want[:65536][~nan[:65536]])      # low half 0: nothing to round
    for n in ew.CAST_LENGTHS:
        assert ew.cast_input(n).numel() == n
    assert ew.CAST_LENGTHS[-1] > ew.CAST_GRID_CAP > ew.CAST_LENGTHS[-2] and ew.CAST_LENGTHS[-2] % 4 == 3


# ================================================================================================ GroupNorm
@pytest.mark.parametrize("case", ew.GN_CASES[:4], ids=str)
def test_groupnorm_bars_accept_the_formula_and_reject_wrong_references(case):
    x, ga, be = ew.gn_input(case)
    B, H, W, C, G = case
    st = ew.gn_stats_restated(x, G)
    m32, r32, sums = ew.gn_stats_one_pass(x, G)
    ex = lambda got, v, a, sl: ew.fp32_excess(got, v, a, sl).max().item()             # noqa: E731
    assert ex(m32, st.mean, st.a_mean, ew.GN_STAT_SLACK) <= 1 and ex(r32, st.rstd, st.a_rstd, ew.GN_STAT_SLACK) <= 1
    # the planted groups: constant (mean exact, var 0, rstd = eps^-1/2) and mean 1000 with spread 1e-2
    assert st.mean[0, 1].item() == ew.GN_CONST and st.var[0, 1].item() == 0 and m32[0, 1].item() == ew.GN_CONST
    assert abs(st.rstd[0, 1].item() * ew.EPS ** 0.5 - 1) < 1e-12
    if H * W > 1:
        assert abs(st.mean[B - 1, G - 1].item() - 1000) < 0.01 and 0.3e-2 < st.var[B - 1, G - 1].item() ** 0.5 < 3e-2
        assert st.a_rstd[B - 1, G - 1] / st.rstd[B - 1, G - 1] > 100 > 1.01 > (st.a_rstd[0, 0] / st.rstd[0, 0]).item()
    for sw, sl in ((False, ew.GN_Y_SLACK), (True, ew.GN_SWISH_SLACK)):
        v, a = ew.gn_apply_restated(x, ga, be, G, st, sw)
        assert ex(ew.gn_apply_fp32(x, ga, be, G, m32, r32, sw), v, a, sl) <= 1
        if not sw:
            assert torch.equal(v[0, :, :, C // G:2 * C // G].float(), be[C // G:2 * C // G].expand(H, W, -1)), "constant group: y == beta"
        wrong, _ = ew.gn_apply_restated(x, ga, be, G, st, sw, wrong_cpg=True)
        assert ex(wrong.float(), v, a, sl) >= 2
    # unbiased variance: 1 / (2 n) of rstd, n <= 2800 here
    wrong = ew.gn_stats_restated(x, G, unbiased=True)
    per = ew.fp32_excess(wrong.rstd.float(), st.rstd, st.a_rstd, ew.GN_STAT_SLACK)
    assert per.max().item() >= 2
    v, a = ew.gn_apply_restated(x, ga, be, G, st, False)
    wst = ew._ns(mean=st.mean, rstd=wrong.rstd, a_rstd=st.a_rstd)
    assert ex(ew.gn_apply_restated(x, ga, be, G, wst, False)[0].float(), v, a, ew.GN_Y_SLACK) >= 2


@pytest.mark.parametrize("case", ew.GN_CASES[:4], ids=str)
def test_groupnorm_integer_input_has_exact_sums(case):
    x = ew.gn_int_input(case)
    G = case[4]
    _, _, sums = ew.gn_stats_one_pass(x, G)
    assert torch.equal(sums, sums.round()) and sums.abs().max().item() < 2 ** 53
    xg = ew.gn_groups(x, G)
    flipped = torch.stack((xg.flip(1).sum((1, 3)), (xg * xg).flip(1).sum((1, 3))), -1)
    assert torch.equal(flipped, sums)


# ================================================================================================ softmax
def test_softmax_bar_rejects_the_scale_dropped():
    for case in ew.SOFTMAX_CASES:
        x = ew.softmax_input(case)
        v, a = ew.softmax_restated(x, 0.125)
        assert ew.softmax_excess(ew.softmax_fp32(x, 0.125), v, a) <= 1
        wrong, _ = ew.softmax_restated(x, 0.125, scale_after=True)
        if case[1] > 1:
            assert ew.softmax_excess(wrong.float(), v, a) >= 2, case
        same, _ = ew.softmax_restated(x, 1.0, scale_after=True)            # at scale 1 there is nothing to misplace
        assert ew.softmax_excess(same.float(), *ew.softmax_restated(x, 1.0)) <= 1
