"""Every kernel form of `ug_gemm_bf16` (and the grouped weight-gradient launch) against the integer matmul, bit for bit.

The operands hold small integers (tests/exact_products.py), so fp32 accumulation is exact in any order and every form -- whatever
its tiling, k-slicing or summation order -- must give `torch.equal` with the CPU reference on the whole output: one wrong element,
one dropped k-chunk, one partial left out of one tile fails.  Forms are reached through `ops.set_gemm_tile_policy`, or, for the
automatic cases, by shapes that satisfy the selection rule in `launch<>` (csrc/gemm_bf16.hip), quoted at each test.

Epilogues, wherever the entry point instantiates them (nt: all; dgrad, wgrad: bf16 and fp32):
  bf16 / bf16 + bias   small-sum regime, expected (ref + bias).to(bfloat16)
  residual             small-sum regime, integer residual, expected resid + ref
  fp32 beta 0 / 1      dense regime, expected ref / prefill + ref (and prefill + 2 ref after a second call)
  fp32 with alpha_dev  dense regime, 3.0 (first write) and 0.5 (accumulating): expected 3 ref / prefill + ref / 2, exact
Operands are stored with padded leading dimensions (garbage in a k-major operand's padding, zero K tail in a row-major one); the
output's columns past N hold a sentinel that must come back untouched.
"""
import pytest
import torch

import exact_products as ep

pytestmark = pytest.mark.gpu

SMALL_EPIS = ("bf16", "bf16_bias", "resid")
DENSE_EPIS = ("f32_beta0", "f32_beta1", "alpha3", "alpha_half_acc")
MODES = ["nt", "dgrad", "wgrad"]


def _ops():
    from unigen_hip import ops
    return ops


def _epis(mode, *, f32=True):
    """the epilogues ug_gemm_bf16 instantiates for a layout"""
    out = ["bf16", "bf16_bias"] + (["resid"] if mode == "nt" else [])
    return out + (list(DENSE_EPIS) if f32 else [])


def _check(dev, shape, mode, policy, epis, reps=1):
    """one shape, one layout, one policy: every requested epilogue `reps` times in a row, each result exact"""
    ops = _ops()
    M, N, K = shape
    ak, bk = ep.LAYOUTS[mode]
    tag = f"{shape} {mode} policy {policy}"
    kw = dict(M=M, N=N, K=K, a_kmajor=ak, b_kmajor=bk)
    ops.set_gemm_tile_policy(policy)
    try:
        small = [e for e in epis if e in SMALL_EPIS]
        if small:
            a, b, bias, ref = ep.problem(M, N, K, "small")
            A, B, bias_d = ep.store(a, ak, dev), ep.store(b, bk, dev), bias.to(dev)
            for e in small:
                for rep in range(reps):
                    if e == "resid":
                        res = ep.int_prefill(M, N, seed=M + N + K)
                        res_d = ep.out_buffer(M, N, torch.float32, dev, prefill=res)
                        out = ep.out_buffer(M, N, torch.float32, dev)
                        ops.gemm(A, B, out=out, epilogue=ops.UG_EPI_RESID, resid=res_d, **kw)
                        ep.assert_exact(out, N, res + ref, f"{tag} residual #{rep}")
                        ep.assert_exact(res_d, N, res, f"{tag} residual input #{rep}")
                    else:
                        out = ep.out_buffer(M, N, torch.bfloat16, dev)
                        ops.gemm(A, B, out=out, bias=bias_d if e == "bf16_bias" else None, **kw)
                        want = ref + bias.float() if e == "bf16_bias" else ref
                        ep.assert_exact(out, N, want.to(torch.bfloat16), f"{tag} {e} #{rep}")
            del A, B
        dense = [e for e in epis if e in DENSE_EPIS]
        if dense:
            a, b, _, ref = ep.problem(M, N, K, "dense")
            A, B = ep.store(a, ak, dev), ep.store(b, bk, dev)
            pre = ep.int_prefill(M, N, seed=M + 2 * N + K)
            for e in dense:
                beta = e in ("f32_beta1", "alpha_half_acc")
                alpha = {"alpha3": 3.0, "alpha_half_acc": 0.5}.get(e)
                alpha_d = None if alpha is None else torch.tensor([alpha], dtype=torch.float32, device=dev)
                out = ep.out_buffer(M, N, torch.float32, dev, prefill=pre)         # (beta 0 overwrites the prefill)
                for rep in range(reps):
                    ops.gemm(A, B, out=out, epilogue=ops.UG_EPI_F32, beta=int(beta), alpha_dev=alpha_d, **kw)
                    scale = (alpha or 1.0) * (rep + 1 if beta else 1)
                    ep.assert_exact(out, N, (pre if beta else 0) + scale * ref, f"{tag} {e} #{rep}")
    finally:
        ops.set_gemm_tile_policy(-1)


# ------------------------------------------------------------------------------------------------ 128 x 128 kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", [0, 2], ids=["two_lds_stages", "one_lds_stage"])
def test_128x128_kernel(dev, policy, mode):
    """`gemm_kernel<EPI, AK, BKM, DBUF>`: policy 0 / 2 skip every other branch of `launch<>` and pin DBUF.  Ragged M, N and K against
    the 128 x 128 x 64 tile; K % 8 != 0 where a k-major operand allows it.  (The accumulating fp32 launch at K = 256 is also cut in
    two along K with atomics: `splits = min(32, 768 / tiles, nk / 2)`.)"""
    shapes = ep.GEMM_128 + (ep.GEMM_128_KMAJOR_ONLY if mode != "nt" else [])
    for shape in shapes:
        _check(dev, shape, mode, policy, _epis(mode))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ep.GEMM_ATOMIC_SPLIT, ids=str)
def test_128x128_atomic_split_along_k(dev, shape, mode):
    """Automatic: `EPI == EPI_F32 && a.beta == 1 && tiles < 384` gives `splits = min(32, 768 / tiles, nk / 2)` = 16 slices for
    (64, 64, 2048) (1 tile, 32 k-tiles) and 8 for (300, 200, 1000) (6 tiles, 16 k-tiles); with 1 and 2 tiles of 256 x 256 none of the
    256-wide forms applies (`p8_fits` needs >= 200 tiles, the private partials >= 24).  Integer-prefilled C, two calls in a row into
    the same C, and the device-scalar alpha on the atomic path."""
    _check(dev, shape, mode, -1, ["f32_beta1", "alpha_half_acc"], reps=2)


# ------------------------------------------------------------------------------------------------ staggered 256 x 256 kernel
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("policy", [103, 105, 3 | 0x100], ids=["one_barrier", "two_barriers", "narrow_epilogue"])
def test_staggered_256x256_kernel(dev, policy, mode):
    """`gemm_kernel_p8` forced (policy 3 and its loop / epilogue bits): whole tiles, ragged M, N, K, all three layouts."""
    shapes = ep.GEMM_STAGGERED + (ep.GEMM_STAGGERED_KMAJOR_ONLY if mode != "nt" else [])
    for shape in shapes:
        _check(dev, shape, mode, policy, _epis(mode))


# ------------------------------------------------------------------------------------------------ 128 ... 320 x 256 kernel
@pytest.mark.parametrize("mode", ["nt", "dgrad"])
@pytest.mark.parametrize("height", ep.P10_HEIGHTS)
def test_p10_forced_tile_height(dev, height, mode):
    """`gemm_kernel_p10<EPI, BKM, F0, F1>` at every instantiated height (policy 32 + h / 16): M = 2 h + 117 leaves a ragged third row
    tile; bf16 (+ bias) for both layouts, the residual epilogue for nt (the kernel has no fp32 or A-k-major form)."""
    _check(dev, ep.p10_shape(height), mode, 32 + height // 16, _epis(mode, f32=False))


@pytest.mark.parametrize("mode", ["nt", "dgrad"])
def test_p10_forced_320_rows(dev, mode):
    _check(dev, ep.GEMM_P10_320, mode, 10, _epis(mode, f32=False))


@pytest.mark.parametrize("mode", ["nt", "dgrad"])
def test_p10_automatic_one_round_choice(dev, mode):
    """Automatic: N % 256 == 0, K % 32 == 0, ldc % 8 == 0 make the shape `aligned`; the loop over heights takes the first with
    `wgs = ceil(M / h) * (N / 256) <= 256` and keeps it `if (wgs >= 64 && !(a.K / PBK >= 2048 && wgs < 200))`: for 12 336 x 1 536
    that is h = 304 (41 x 6 = 246 workgroups; 288 rows would need 258)."""
    _check(dev, ep.GEMM_P10_AUTO, mode, -1, _epis(mode, f32=False))


# ------------------------------------------------------------------------------------------------ k-sliced forms
@pytest.mark.parametrize("mode", MODES)
def test_k_sliced_tail_with_tail_finish(dev, mode):
    """Policy 6: 17 x 16 = 272 tiles of 256 x 256 = one round + 16 leftover tiles, each cut into 2 k-slices (82 k-tiles: `while (sp > 1
    && nk32 / sp < 40) --sp` stops at 2, which policy 6 admits) whose partials `tail_finish_kernel` sums under the launch's epilogue.
    Every layout and epilogue, alpha_dev included, each twice: the second launch reuses the handle's scratch."""
    _check(dev, ep.GEMM_TAIL, mode, 6, _epis(mode), reps=2)


@pytest.mark.parametrize("policy", [8, -1], ids=["policy_8", "auto"])
def test_every_tile_cut_along_k_weight_gradient(dev, policy):
    """`EPI == EPI_F32 && tiles_p8 >= 24 && tiles_p8 <= 128 && a.M >= 512 && a.N >= 512`: 6 x 5 = 30 tiles, `sp = 256 / 30 = 8`
    reduced to 2 by `while (sp > 1 && nk32 / sp < 32) --sp` (66 k-tiles); taken under policy 8 and automatically.  Weight-gradient
    layout, K % 8 != 0, accumulating twice; first write and alpha as well."""
    _check(dev, ep.GEMM_PRIVATE_WGRAD, "wgrad", policy, ["f32_beta1", "alpha_half_acc", "f32_beta0", "alpha3"], reps=2)


def test_every_tile_cut_along_k_long_contraction(dev):
    """`tiles_p8 >= 24 && tiles_p8 < 200 && nk32 >= 2048`: 6 x 6 = 36 tiles, 2 048 k-tiles, 7 slices (252 of 256 workgroups is the
    fullest round); dgrad layout, bf16 epilogue from the summing pass.  N % 256 != 0 keeps the 128 ... 320-row kernel out.  Under
    policy 8 and automatically, the automatic launch twice."""
    _check(dev, ep.GEMM_PRIVATE_LONG, "dgrad", 8, ["bf16_bias"])
    _check(dev, ep.GEMM_PRIVATE_LONG, "dgrad", -1, ["bf16", "bf16_bias"], reps=2)


# ------------------------------------------------------------------------------------------------ grouped weight gradients
def test_wgrad_group(dev):
    """`ug_gemm_bf16_wgrad_group`: five problems in one grid (the second with a contraction length of its own), beta alternating,
    padded leading dimensions with garbage in the operands' padding and a sentinel in the outputs'."""
    ops = _ops()
    probs, wants, bufs = [], [], []
    for n, (rows, cols) in enumerate(ep.WGRAD_GROUP_SHAPES):
        dy, x, _, ref = ep.problem(rows, cols, ep.wgrad_group_k(n), "dense")
        beta = n % 2
        pre = ep.int_prefill(rows, cols, seed=n)
        buf = ep.out_buffer(rows, cols, torch.float32, dev, prefill=pre, align=4)
        probs.append((ep.store(dy, True, dev), ep.store(x, True, dev), buf[:, :cols], beta))
        wants.append(pre + ref if beta else ref)
        bufs.append(buf)
    old = ops.WGRAD_GROUP_MIN_TILES
    ops.WGRAD_GROUP_MIN_TILES = 0
    try:
        ops.gemm_wgrad_group(probs)
    finally:
        ops.WGRAD_GROUP_MIN_TILES = old
    for n, (buf, want) in enumerate(zip(bufs, wants)):
        ep.assert_exact(buf, want.shape[1], want, f"wgrad group problem {n} {tuple(want.shape)}")
