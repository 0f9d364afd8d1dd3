"""Restatements for the text pick kernels (include/unigen_hip.h: ug_text_pick, ug_text_sample), beside truncation_ref.py:

  StopRule          the record and stop rule of models/unigen.py: emit_until_stop, one step at a time, in plain Python;
  sorted_draw_ok    float64 check of an inverse-CDF draw over the kept entries ordered by value descending, index ascending."""
import torch

import truncation_ref as ref


class StopRule:
    """Per row: a finished row emits pad_id (when there is one); token i is recorded; a row finishes on its first stop id
    (lengths[r] = i + 1); steps_used = i + 1 of the step at which the last row finished (0: not yet)."""

    def __init__(self, rows, nsteps, stop_ids=(), pad_id=None):
        self.stop, self.pad = [int(s) for s in stop_ids], pad_id
        self.done = [0] * rows
        self.lengths = [nsteps] * rows
        self.remaining, self.steps_used, self.step = rows, 0, 0
        self.out = [[0] * nsteps for _ in range(rows)]

    def emit(self, picked):
        """picked: the rows' raw picks of this step -> the tokens recorded and fed back"""
        fed = []
        for r, p in enumerate(picked):
            tok = int(self.pad) if self.done[r] and self.pad is not None and self.pad >= 0 else int(p)
            self.out[r][self.step] = tok
            if tok in self.stop and not self.done[r]:
                self.lengths[r] = self.step + 1
                self.done[r] = 1
                self.remaining -= 1
                if self.remaining == 0:
                    self.steps_used = self.step + 1
            fed.append(tok)
        self.step += 1
        return fed


def sorted_draw_terms(v, t, token):
    """float64 (above, j, e, T) of `token` among the kept entries {v >= t}: mass of the strictly greater kept values, its rank among
    the equal kept values in index order, its own mass, the kept mass"""
    keep = v >= t
    ex = torch.exp(v - v.max())
    T = float(ex[keep].sum())
    g = int(token)
    above = float(ex[keep & (v > v[g])].sum())
    j = int((v[:g] == v[g]).sum())
    return above, j, float(ex[g]), T


def sorted_draw_ok(v, t, token, u, d=ref.D):
    """is `token` a legitimate inverse-CDF draw on u over {v >= t} in the order value descending, index ascending?  It must be kept and
    above + j e - d T <= u T < above + (j + 1) e + d T"""
    if not bool(v[int(token)] >= t):
        return False
    above, j, e, T = sorted_draw_terms(v, t, token)
    return above + j * e - d * T <= float(u) * T < above + (j + 1) * e + d * T
