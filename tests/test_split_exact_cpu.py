"""The conditions that tests/test_split_exact_gpu.py rests on, checked for every listed case without a GPU (tests/split_exact.py):
exactness of every regime, second-plane coverage of the two-plane regimes, the kernel each shape selects, and that a reference
which misses one product, one tap, one slab or the zero border is rejected by `torch.equal`."""
import copy
import math

import pytest
import torch

import split_exact as sx


def test_split_construction_at_k_1152():
    """The two-plane operand under the kernel's own split at K = 1152: a quarter of the entries carry a second plane of +1 unit (4095:
    -1), the planes add back to the operand exactly, the integer partner has no second plane, and an fp32 accumulation in the
    kernel's product order (w1 x2 first, then w2 x1 and w1 x1 alternating, k ascending) equals the float64 contraction."""
    K, M, N = 1152, 24, 20
    x, w = sx.two_plane((M, K), 7), sx.small_ints((N, K), 8)
    big = x.abs() > 2048
    assert ((x[big].abs() % 2) == 1).all() and (x[big].abs() < 4096).all() and (x == 4095).sum().item() == 1
    assert (x[~big].abs() <= 4).all() and (x != 0).all()
    x1, x2, ex = sx.split_planes(x)
    w1, w2, ew = sx.split_planes(w)
    assert ex == 14 - math.floor(math.log2(4095.0)) == 3 and ew == 13
    assert torch.equal((x1.double() + x2.double()) / 8.0, x.double())
    assert torch.equal(x2 != 0, big) and 0.2 < big.float().mean().item() < 0.3
    assert set(x2[big].unique().tolist()) == {-8.0, 8.0} and (x2 == -8.0).sum().item() == 1            # +1 unit except below 4095
    assert not w2.any() and set(w.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    # twelve significant bits: the scaled value is no f16
    assert not torch.equal(x1[big], (x * 8.0)[big])
    bound = ((x1.abs() + x2.abs()) @ w1.abs().t()).max().item() * 2.0 ** -(ex + ew)
    print(f"    K = 1152: max sum (|x1| + |x2|) |w| = {bound / sx.EXACT_LIMIT:.4f} * 2^24")
    assert bound < 0.1 * sx.EXACT_LIMIT, bound / sx.EXACT_LIMIT
    ref = x.double() @ w.double().t()
    acc = torch.zeros(M, N, dtype=torch.float32)
    for k0 in range(0, K, 32):                               # one slab of mma_slab per step, fp32 throughout
        for k in range(k0, k0 + 32):
            acc = acc + x2[:, k:k + 1] * w1[:, k].unsqueeze(0)
        for k in range(k0, k0 + 32):
            acc = acc + x1[:, k:k + 1] * w2[:, k].unsqueeze(0)
            acc = acc + x1[:, k:k + 1] * w1[:, k].unsqueeze(0)
    assert torch.equal((acc * 2.0 ** -(ex + ew)).double(), ref)


@pytest.mark.parametrize("name,regime", sx.CONV_PARAMS + sx.LINEAR_PARAMS)
def test_case_conditions_coverage_and_rejections(name, regime):
    """exactness conditions (asserted while the problem is built), second-plane share >= 10 % and presence in every (tap, slab), the
    loose bound, and the rejected references"""
    if name in sx.CONV_BY_NAME:
        p = sx.conv_problem(name, regime)
        c = p.case
    else:
        p = copy.copy(sx.linear_problem(name, regime))
        c = p.case = sx.linear_as_case(p.case)
    cond = p.cond
    assert cond.loose_ok and cond.ratio < 1.0
    if regime == "int":
        assert cond.share_x2 == 0.0 and cond.share_w2 == 0.0
    elif regime == "x2":
        assert cond.share_x2 >= 0.10 and cond.share_w2 == 0.0
        assert (sx.slab_coverage(cond.x2, "x") > 0).all()
    else:
        assert cond.share_w2 >= 0.10 and cond.share_x2 == 0.0
        assert (sx.slab_coverage(cond.w2, "w") > 0).all()
    rej = sx.rejected_variants(p)
    flags = {k: v for k, v in rej.items() if not k.startswith("share")}
    assert flags and all(flags.values()), {k: v for k, v in flags.items() if not v}
    assert sum(k.startswith("without tap") for k in flags) >= 1 and sum(k.startswith("without slab") for k in flags) >= 1
    if c.entry != "f32":
        assert "without w1x1" in flags
        if regime == "x2":
            assert "without w1x2" in flags
        if regime == "w2":
            assert "without w2x1" in flags
    print(f"    {name:18s} {regime:3s} x2 {cond.share_x2:.3f} w2 {cond.share_w2:.3f} sum|x||w| {cond.ratio:.4f} * 2^24  " +
          " ".join(f"{k[6:]} {v:.3f}" for k, v in rej.items() if k.startswith("share")))


def test_every_product_is_missed_everywhere_in_some_regime():
    """For each of w1 x2, w2 x1 and w1 x1 there is a regime in which a reference without that product differs from the true one in
    EVERY output element (K = 1152, 70 x 132 outputs): the cross terms are positive everywhere by construction."""
    table = {}
    for regime in sx.REGIMES:
        p = copy.copy(sx.linear_problem("split_lin_k1152", regime))
        p.case = sx.linear_as_case(p.case)
        rej = sx.rejected_variants(p, nsub=p.case.Cout)
        for prod in ("w1x2", "w2x1", "w1x1"):
            table[(prod, regime)] = rej.get("share " + prod, 0.0)
    print("    share of outputs that differ without the product (int, x2, w2): " +
          "; ".join(f"{prod}: " + " ".join(f"{table[(prod, r)]:.4f}" for r in sx.REGIMES) for prod in ("w1x2", "w2x1", "w1x1")))
    for prod in ("w1x2", "w2x1", "w1x1"):
        assert max(table[(prod, r)] for r in sx.REGIMES) == 1.0, (prod, table)
    assert table[("w1x2", "x2")] == 1.0 and table[("w2x1", "w2")] == 1.0


def test_stated_kernels_and_every_instantiation_selected():
    """the kernel written next to each case is what the restated launcher conditions select, and every instantiation is reached"""
    seen = set()
    for c in sx.CONV_CASES:
        assert sx.case_kernel(c) == c.kernel, (c.name, sx.case_kernel(c))
        seen.add(c.kernel)
    for g in sx.GEMM_CASES:
        assert sx.gemm_kernel(g) == g.kernel, (g.name, sx.gemm_kernel(g))
        seen.add(g.kernel)
    for c in sx.LINEAR_CASES:
        assert sx.linear_kernel(c) == c.kernel, (c.name, sx.linear_kernel(c))
        seen.add(c.kernel)
    missing = [k for k in sx.IGEMM_ALL + sx.SPLIT_ALL if k not in seen]
    assert not missing, missing
    # the shapes the issue names: ragged slabs, Cout = 4 x odd, a tile that crosses images, a grid rounded up to 8 tiles
    by = sx.CONV_BY_NAME
    assert by["split_k1_ragged"].Cin % 32 == 4 and by["split_up_ragged"].Cin % 32 == 4 and (by["split_k3"].Cout // 4) % 2 == 1
    c = by["split_k1_ragged"]
    hw = c.H * c.W
    assert hw < 128 < 2 * hw and (c.B * hw) % 128 != 0
    real, launched = sx.split_grid_x(c.B * hw)
    assert launched > real
    assert sx.split_grid_x(128 * 128) == (128, 128)
    for name in ("split_stats", "split_wide_stats", "patch_stats", "patch16_stats"):
        assert by[name].Cout % 128 == 64                                    # a partial 128-channel block in every statistics case
    # M straddling a 128-row tile and M below one, on the fp32 kernel
    ms = {c.name: c.B * math.prod(sx.out_hw(c)) for c in sx.CONV_CASES if c.entry == "f32"}
    assert ms["f32_siglip_patch"] == 12 and ms["f32_13_512"] == 99 and ms["f32_4_128"] == 198
    assert any(g.M < 128 for g in sx.GEMM_CASES) and any(128 < g.M < 256 for g in sx.GEMM_CASES)


@pytest.mark.parametrize("name", [g.name for g in sx.GEMM_CASES])
def test_gemm_problems_are_exact(name):
    p = sx.gemm_problem(name)
    g = p.case
    live = (p.c_expect != sx.SENTINEL).sum().item()
    assert live <= max(g.outer, 1) * g.inner * g.M * g.N and live > 0.9 * max(g.outer, 1) * g.inner * g.M * g.N
    assert (p.c_expect[-sx.GUARD:] == sx.SENTINEL).all()
    assert math.log2(g.alpha) == round(math.log2(g.alpha))


def test_weight_image_expectation():
    """the expected split weight image of a ragged Cin and cout_pad > Cout: zero planes in the padding, exact reconstruction"""
    wi = sx.WEIGHT_IMAGE
    w = sx.two_plane((wi["Cout"], wi["Cin"], 3, 3), 5)
    wp = sx.pack_weight(w, wi["cout_pad"])
    planes, ew = sx.weight_image_expect(wp)
    assert planes.shape == (9, 2, 2, 2, 128, 32)
    assert not planes[:, 1, :, :, :, 4:].any() and not planes[:, :, 1].any() and not planes[:, :, 0, :, wi["Cout"]:].any()
    back = planes.double().sum(dim=3) * 2.0 ** -ew                            # [tap, slab, nblk, row, c]
    back = back.permute(0, 1, 4, 2, 3).reshape(9, 64, wi["cout_pad"])[:, :wi["Cin"]]
    assert torch.equal(back, wp.double()) and (planes[:, :, :, 1] != 0).float().mean().item() > 0.01


@pytest.mark.parametrize("B,T,H,hd", sx.ATTN_SHAPES)
def test_attention_regimes(B, T, H, hd):
    """the select regime's margin conditions (asserted while the problem is built) and its key coverage; the uniform regime"""
    for v_regime in ("int", "x2"):
        p = sx.attn_select_problem(B, T, H, hd, v_regime)
        assert 32.0 <= p.margin < 64.0 and p.G == 2.0 ** round(math.log2(p.G))
        assert (p.sel == 0).any() and (p.sel == T - 1).any()
        assert (p.share_v2 > 0.1) == (v_regime == "x2")
        # a softmax in float64 puts all but 2^-39 of the weight on the selected key
        D = H * hd
        q = p.qkv[:, :D].view(B, T, H, hd).permute(0, 2, 1, 3).double()
        k = p.qkv[:, D:2 * D].view(B, T, H, hd).permute(0, 2, 1, 3).double()
        pr = torch.softmax(p.scale * q @ k.transpose(-1, -2), dim=-1)
        assert (pr.gather(-1, p.sel[..., None]) > 1 - 2.0 ** -39).all()
    u = sx.attn_uniform_problem(B, T, H, hd)
    assert u.exact == (T == 64)
