"""Plain-Python statement of the token rules of prompt-lookup speculative decoding (include/unigen_hip.h: ug_spec_verify, rules (b) to
(e); csrc/spec_plan.h states the same for the kernel).  Shared by test_spec_ref_cpu.py (against transformers' candidate generator and the
header's host program) and test_spec_verify_gpu.py (against the kernel)."""


def accept(g, tok, n_draft):
    """(b) the number of leading s < n_draft with g[s] == tok[s + 1]"""
    a = 0
    while a < n_draft and g[a] == tok[a + 1]:
        a += 1
    return a


def emit(g, a, stop_ids, emitted, width):
    """(c) g[0 .. a] cut after the first stop id (inclusive) and at `width` -> (tokens emitted, done)"""
    out, done = [], False
    for t in g[:a + 1]:
        if emitted + len(out) >= width:
            break
        out.append(t)
        if t in stop_ids:
            done = True
            break
    return out, done or emitted + len(out) >= width


def draft(h, G, K):
    """(d) the ids behind the earliest earlier occurrence of the last G' ids of h, for the largest G' <= min(G, len(h) - 1) that has one;
    at most K of them, never past the end of h.  [] without a match."""
    n = len(h)
    for g in range(min(G, n - 1), 0, -1):
        for i in range(0, n - g):                       # i + g < n: at least one id behind the window
            if h[i:i + g] == h[n - g:]:
                return h[i + g:min(i + g + K, n)]
    return []


class SpecRef:
    """The state ug_spec_verify keeps, advanced by the picks of one call."""

    def __init__(self, history, S, G, K, width, stop_ids=(), pos=0):
        self.h, self.S, self.G, self.K, self.width, self.stop = list(history), S, G, K, width, set(stop_ids)
        self.out, self.done, self.steps, self.drafted, self.accepted = [], False, 0, 0, 0
        self.n_draft, self.tok, self.pos, self.length = 0, None, pos, None

    def verify(self, g, tok, advance=True):
        """g: the picks of the call's rows; tok: the step's input tokens (list of S).  -> the next tok (list of S), or None when the
        call changed neither tok nor x (the session is finished, now or before)"""
        if self.done:
            return None
        nd = min(self.n_draft, len(g) - 1)
        a = accept(g, tok, nd)
        new, done = emit(g, a, self.stop, len(self.out), self.width)
        self.out += new
        self.h += new
        if advance:
            self.steps, self.drafted, self.accepted = self.steps + 1, self.drafted + nd, self.accepted + a
            self.pos += len(new)
        if done:
            self.done, self.length = True, len(self.out)
            return None
        d = draft(self.h, self.G, self.K) if self.K > 0 else []
        self.n_draft = len(d)
        nxt = [new[-1]] + d
        self.tok = nxt + [nxt[-1]] * (self.S - len(nxt))       # padding rows repeat the last valid one
        return self.tok
