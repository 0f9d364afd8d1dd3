"""Fused AdamW over flat parameter runs (replaces torch.optim.AdamW.step at reference
training/train.py:324-330,780; same constructor / param-group interface, same update rule).

Parameters that are adjacent views of one buffer (the UniGen backbone's flat fp32 master/grad
buffers) are merged into runs, so a 1.56 B-parameter step is a few dozen launches of one
HBM-bound kernel instead of one launch per tensor."""
import math

import torch

from . import ops


class _Run:
    __slots__ = ("params", "p_ptr", "numel", "m", "v", "group")


# ------------------------------------------------------------------------------------ gradient-norm clipping
# Replaces torch.nn.utils.clip_grad_norm_ (what accelerator.clip_grad_norm_ calls, reference training/train.py:777) for fp32
# gradients in GPU memory: one read pass for the norm, the clip coefficient left on the device, and either an in-place scale by
# that device scalar -- which returns at once on a step that does not clip -- or no rewrite at all (FusedAdamW takes the factor).
def group_spans(triples):
    """[(storage id, byte address, fp32 count)] -> [(byte address, fp32 count)], sorted, with two tensors merged only where they
    lie in ONE storage and the second starts exactly where the first ends.  FusedAdamW._build_runs bridges gaps of up to 1 KB
    because updating padding is harmless; reading padding into a norm is not, so nothing is bridged here.  (The backbone's flat
    gradient buffer still comes out as one span today: FlatParams pads every tensor to 64 elements, and every shape in it is a
    multiple of 64 already because hidden and intermediate sizes must be -- a convenience this function does not rely on.)"""
    spans = []
    for sid, addr, n in sorted((int(s), int(a), int(n)) for s, a, n in triples):
        if n <= 0:
            continue
        if spans and spans[-1][0] == sid and spans[-1][1] + 4 * spans[-1][2] == addr:
            spans[-1][2] += n
        else:
            spans.append([sid, addr, n])
    return [(a, n) for _, a, n in spans]


class _ClipPlan:
    """Span table and partial buffer of one set of gradient tensors (device memory, built once per set)."""
    __slots__ = ("table", "partials", "blocks")


_PLANS = {}             # (device index, ((storage address, data address, numel), ...)) -> _ClipPlan
_PLANS_MAX = 16


def _fusable(g):
    return g.is_cuda and g.dtype == torch.float32 and g.layout == torch.strided and g.is_contiguous() and g.data_ptr() % 4 == 0


def _plan_for(grads):
    key = (grads[0].device.index, tuple((g.untyped_storage().data_ptr(), g.data_ptr(), g.numel()) for g in grads))
    plan = _PLANS.get(key)
    if plan is None:
        if len(_PLANS) >= _PLANS_MAX:
            _PLANS.pop(next(iter(_PLANS)))
        spans = group_spans(key[1])
        if len(spans) > 65535:
            raise ops._l.UniGenHipError("clip_grad_norm_: more than 65535 separate gradient spans")
        plan = _ClipPlan()
        dev = grads[0].device
        plan.table = torch.tensor(spans, dtype=torch.int64).reshape(-1, 2).to(dev)
        plan.blocks = ops.SUMSQ_BLOCKS
        plan.partials = torch.zeros(plan.blocks + 1, dtype=torch.float64, device=dev)       # (+ 1: the slot of the gradients torch handles)
        _PLANS[key] = plan
    return plan


def _split_grads(grads):
    """-> (fused, others): fp32 contiguous dense GPU gradients on one device | everything else (torch's own kernels)"""
    fused, others, dev = [], [], None
    for g in grads:
        if _fusable(g) and (dev is None or g.device == dev) and g.numel() > 0:
            dev = g.device
            fused.append(g)
        else:
            others.append(g)
    return fused, others


def _by_device_and_dtype(grads):
    out = {}
    for g in grads:
        out.setdefault((g.device, g.dtype, g.layout), []).append(g)
    return out


def _norm_into(block, fused, others, max_norm, grad_scale=1.0):
    """Launch the sum of squares over `fused`, add the squared norms torch computes for `others`, finish into `block` (fp32 [8]
    on the gradients' device: norm, coefficient, grad_scale * coefficient, non-finite flag, fp64 sum).  Current stream, no sync."""
    for ref in list(ops.BF16_MIRRORS):                     # gradients of a flat buffer: behind an overlapped optimizer update
        o = ref()                                          # (backward already waited for it; this is a None check)
        if o is not None:
            o.wait_pending_update()
    plan = _plan_for(fused)
    with torch.cuda.device(block.device):
        ops.sumsq_spans(plan.table, plan.partials, plan.blocks)
        n_part = plan.blocks
        if others:
            norms = []
            for gs in _by_device_and_dtype(others).values():
                if gs[0].layout == torch.strided:
                    norms += torch._foreach_norm(gs, 2.0)
                else:
                    norms += [torch.linalg.vector_norm(g.coalesce().values(), 2.0) for g in gs]
            plan.partials[plan.blocks:].copy_((torch.stack([n.to(block.device, torch.float64) for n in norms]) ** 2).sum())
            n_part += 1
        ops.clip_finish(plan.partials, n_part, max_norm, block, grad_scale)
    return plan


def _check_max_norm(max_norm, what="max_norm", negative_ok=True):
    max_norm = float(max_norm)
    if math.isnan(max_norm) or (max_norm < 0 and not negative_ok):
        raise ValueError(f"{what} must be a {'' if negative_ok else 'non-negative '}number, got {max_norm}")
    return max_norm


_NONFINITE = ("The total norm of order {} for gradients from `parameters` is non-finite, so it cannot be clipped. To disable "
              "this error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, defer_to=None):
    """torch.nn.utils.clip_grad_norm_'s signature, semantics and return value (a 0-dim fp32 tensor on the gradients' device).

    Contiguous fp32 GPU gradients go through one sum-of-squares launch over their spans, one finish launch and one scale launch
    that reads the coefficient from the device and returns at once when it is exactly 1.0; nothing synchronises with the host
    unless error_if_nonfinite=True.  Other gradients (another dtype, CPU, non-contiguous, sparse) take torch's `_foreach_norm`
    / `_foreach_mul_` and their squared norm joins the fused sum before the finish.  norm_type != 2, or no gradient that
    qualifies, is torch's function unchanged.

    defer_to=<FusedAdamW>: compute the norm, hand the factor to that optimizer's next step() and leave every `.grad` unscaled
    (the returned scalar is then a view of the optimizer's result block, valid until its next norm: clone it to keep it; the
    step's own grad_scale multiplies on top of the factor)."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    max_norm = _check_max_norm(max_norm)
    grads = [p.grad for p in parameters if p.grad is not None]
    fused, others = _split_grads(grads) if float(norm_type) == 2.0 else ([], grads)
    if not fused:
        if defer_to is not None:
            raise ops._l.UniGenHipError("clip_grad_norm_(defer_to=...): no fp32 GPU gradient to take the norm of")
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)
    if defer_to is not None:
        block = defer_to._clip_block_for(fused[0].device)
    else:
        block = torch.empty(8, dtype=torch.float32, device=fused[0].device)       # fresh per call: the returned scalar is a view of it
    plan = _norm_into(block, fused, others, max_norm)
    if error_if_nonfinite and bool(block[3].item()):
        raise RuntimeError(_NONFINITE.format(norm_type))
    if defer_to is not None:
        defer_to._deferred_factor = block[2:3]
        defer_to.last_grad_norm = block[0]
        return block[0]
    ops.scale_spans_(plan.table, block[1:2])
    for (dev, _, layout), gs in _by_device_and_dtype(others).items():
        coef = block[1].to(dev)
        if layout == torch.strided:
            torch._foreach_mul_(gs, coef)
        else:
            for g in gs:
                g.mul_(coef)
    return block[0]


class FusedAdamW(torch.optim.Optimizer):
    """State layout = torch.optim.AdamW's: `self.state[p]` holds `step`, `exp_avg`, `exp_avg_sq` per parameter, so
    `state_dict()` / `load_state_dict()` (what the reference checkpoints through `accelerator.save_state` and
    utils/checkpoint.py:67-69) interoperate with torch.optim.AdamW.  The moment tensors are views of one buffer per
    flat run, which is what the kernel walks."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, overlap=False, max_grad_norm=None):
        """overlap=True: the update of the backbone's flat buffers (HBM-bound, ~9 ms for 1.56 B parameters) is issued on a
        side stream, so whatever the caller runs next that does not touch the backbone -- the frozen MAGVITv2 tokenisation
        of the next batch is MFMA-bound and comes first in every training script -- runs beside it.  The engine makes its own
        streams wait for the update before the first read or write of weights / gradients (embedding lookup, refresh of the
        bf16 copies, gradient clearing, state_dict); code that reads backbone parameters or gradients through plain torch
        ops between step() and the next forward must call `synchronize()` first.  Ordinary parameters (mm_projector, ...)
        are always updated on the current stream.

        max_grad_norm=<float>: step() clips by the global L2 norm of all its groups' gradients (times grad_scale) the way
        torch.nn.utils.clip_grad_norm_ would, without rewriting them: one read pass for the norm, and the update kernels take
        the factor from device memory (ug_adamw_flat_dev), so `.grad` stays unscaled and nothing synchronises with the host.
        `last_grad_norm` is the device scalar of the last step (a view of the optimizer's result block: clone it to keep it past
        the next step).  None (the default): today's behaviour exactly."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, "max_grad_norm", negative_ok=False)
        self.last_grad_norm = None
        self._clip_block = None
        self._deferred_factor = None               # set by clip_grad_norm_(defer_to=self): the next step() applies it
        self._runs = None
        self._step = 0
        self.overlap = bool(overlap)
        self.overlap_blocks = 256                  # one small workgroup per CU: the overlapped update yields registers / LDS
        self._side = None
        self._pending = None

    def synchronize(self):
        """Make the current stream wait for an overlapped update still in flight."""
        if self._pending is not None:
            torch.cuda.current_stream().wait_event(self._pending)
            self._pending = None

    def _clip_block_for(self, device):
        """The optimizer's ONE result block of ug_clip_finish.  With overlap=True the side stream reads the factor out of it
        after the main stream wrote it, so the next write has to stay behind that read.  Of the two ways to get there -- two
        alternating blocks, or ordering the next write behind `_pending` -- this is the second: the current stream waits for
        the update in flight before the next finish is launched on it.  Safe because the update recorded in `_pending` is the
        only reader on another stream and every other reader is on the writing stream; free because the forward and backward
        that produced the gradients being normed already waited for the same event.  The block lives as long as the optimizer."""
        if self._clip_block is None or self._clip_block.device != device:
            self._clip_block = torch.zeros(8, dtype=torch.float32, device=device)
        self.synchronize()
        return self._clip_block

    def zero_grad(self, set_to_none=True):
        if not set_to_none:
            self.synchronize()                     # an in-place clear would race with the update reading the gradients
        return super().zero_grad(set_to_none=set_to_none)

    def state_dict(self):
        self.synchronize()
        return super().state_dict()

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._runs = None                          # rebuilt (moments carried over from self.state) at the next step

    def _build_runs(self):
        runs = []
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.requires_grad]
            for p in ps:
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                    raise ops._l.UniGenHipError("FusedAdamW needs contiguous fp32 parameters in GPU memory")
            ps.sort(key=lambda t: t.data_ptr())
            cur = None
            for p in ps:
                end = None if cur is None else cur.p_ptr + cur.numel * 4
                same_store = cur is not None and cur.params[-1].untyped_storage().data_ptr() == p.untyped_storage().data_ptr()
                if cur is not None and same_store and 0 <= p.data_ptr() - end <= 1024 and (p.data_ptr() - cur.p_ptr) % 16 == 0:
                    cur.params.append(p)
                    cur.numel = (p.data_ptr() - cur.p_ptr) // 4 + p.numel()
                else:
                    cur = _Run()
                    cur.params, cur.p_ptr, cur.numel, cur.group = [p], p.data_ptr(), p.numel(), gi
                    runs.append(cur)
        for r in runs:
            dev = r.params[0].device
            r.m = torch.zeros(r.numel, dtype=torch.float32, device=dev)
            r.v = torch.zeros(r.numel, dtype=torch.float32, device=dev)
            for p in r.params:
                o = (p.data_ptr() - r.p_ptr) // 4
                m, v = r.m[o:o + p.numel()].view_as(p), r.v[o:o + p.numel()].view_as(p)
                old = self.state.get(p)
                if old:                            # loaded checkpoint / earlier run layout: carry the moments over
                    m.copy_(old["exp_avg"])
                    v.copy_(old["exp_avg_sq"])
                    self._step = max(self._step, int(float(old.get("step", 0))))
                self.state[p] = {"step": torch.tensor(float(self._step)), "exp_avg": m, "exp_avg_sq": v}
        self._runs = runs

    def load_state_dict(self, state_dict):
        """torch.optim.AdamW layout in (from this class or from torch.optim.AdamW); the loaded moments are copied into the
        flat run buffers and the single bias-correction step count resumes from the stored one."""
        super().load_state_dict(state_dict)
        self._step = 0
        self._runs = None
        with torch.no_grad():
            self._build_runs()

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = closure() if closure is not None else None
        if self._runs is None:
            self._build_runs()
        self._step += 1
        lib = ops._l.api()
        factor, host_scale = None, float(grad_scale)
        if self._deferred_factor is not None:      # clip_grad_norm_(..., defer_to=self) took the norm already
            factor, self._deferred_factor = self._deferred_factor, None
        elif self.max_grad_norm is not None:
            grads = [p.grad for g in self.param_groups for p in g["params"] if p.requires_grad and p.grad is not None]
            fused, others = _split_grads(grads)
            if fused:
                block = self._clip_block_for(fused[0].device)
                _norm_into(block, fused, others, self.max_grad_norm, host_scale)
                factor, host_scale = block[2:3], 1.0         # word [2] = grad_scale * clip coefficient
                self.last_grad_norm = block[0]
        # masters whose bf16 compute mirror is in sync right now stay in sync: the kernel writes the mirror too
        synced = {}
        main = torch.cuda.current_stream()
        side_used = False
        for r in self._runs:
            g = self.param_groups[r.group]
            first = r.params[0]
            if first.grad is None:
                if any(p.grad is not None for p in r.params):
                    raise ops._l.UniGenHipError("FusedAdamW: partially missing gradients inside a flat run")
                continue
            g_ptr = first.grad.data_ptr()
            for p in r.params[1:]:
                if p.grad is None or p.grad.data_ptr() - g_ptr != p.data_ptr() - r.p_ptr:
                    raise ops._l.UniGenHipError("FusedAdamW: gradient views do not mirror the parameter layout")
            b1, b2 = g["betas"]
            owner, mirror = ops.find_bf16_mirror(r.p_ptr, r.numel)
            if owner is not None:
                if id(owner) not in synced:
                    synced[id(owner)] = (owner, owner._seen_version == owner.master._version)
                if not synced[id(owner)][1]:
                    mirror = 0
            stream = main
            if self.overlap and owner is not None:          # flat backbone buffers only: every reader goes through the engine
                if self._side is None:
                    self._side = torch.cuda.Stream()
                if not side_used:
                    self._side.wait_stream(main)
                    side_used = True
                stream = self._side
            max_blocks = self.overlap_blocks if stream is not main else 0
            if factor is None:
                lib.ug_adamw_flat(r.p_ptr, g_ptr, r.m.data_ptr(), r.v.data_ptr(), mirror, r.numel, float(g["lr"]), b1, b2,
                                  g["eps"], g["weight_decay"], self._step, host_scale, max_blocks, stream.cuda_stream)
            else:
                lib.ug_adamw_flat_dev(r.p_ptr, g_ptr, r.m.data_ptr(), r.v.data_ptr(), mirror, r.numel, float(g["lr"]), b1, b2,
                                      g["eps"], g["weight_decay"], self._step, host_scale, factor.data_ptr(), max_blocks,
                                      stream.cuda_stream)
            # the kernel wrote through a raw pointer: bump the (shared) version counter so the engine
            # knows its bf16 compute copies are stale
            torch.autograd.graph.increment_version(first)
        if side_used:
            ev = torch.cuda.Event()
            ev.record(self._side)
            self._pending = ev
            for owner, _ in synced.values():
                owner.pending_update = ev
        for owner, ok in synced.values():
            if ok:
                owner._seen_version = owner.master._version
        for st in self.state.values():
            st["step"].fill_(float(self._step))
        return loss
