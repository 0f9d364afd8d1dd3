"""Beam search bookkeeping of the text loop: which candidates become the next running beams, which enter the finished pool, when a
call is over and what it returns.  Pure torch on small host tensors -- no engine, no kernel calls -- so it runs anywhere; the per-step
candidates come from outside (on the GPU: ops.beam_candidates; in the CPU suite: tests/beam_ref.py).

The rule is stated once, in include/unigen_hip.h under "Beam search of the text loop": transformers' GenerationMixin._beam_search with
do_sample=False.  The arithmetic is kept in fp32 tensors and in the order transformers uses (the -1e9 masks are ADDED, the length
penalty divides by a Python float), so that scores agree to the rounding of the candidates themselves."""
import torch

DEAD = -1.0e9                     # transformers' mask value: added to a score to take it out of every later top-k


def beams_to_keep(num_beams, n_eos):
    """K: candidates per group and step, enough that num_beams of them are no eos token"""
    return max(2, 1 + int(n_eos)) * int(num_beams)


class BeamSearch:
    """State of one beam search call over `groups` prompts of `num_beams` beams (rows g * num_beams + b of the decode state).

    step(cand_score, cand_beam, cand_token) consumes one step's [groups, K] candidates (descending; slots the live beams could not
    fill hold (-inf, -1, -1)) and returns (parent int32 [R]: the absolute row each next running beam continues, token int64 [R, 1]:
    the token it appends, finished: whether the call is over).  It makes one device-to-host read, of the candidates.
    running_scores(): fp32 [R], the next step's beam scores.  finalize(): (sequences long [groups * n, new], scores fp32 [groups * n]),
    each prompt's num_return_sequences best hypotheses, best first, padded behind their end with pad_id and cut at the longest."""

    def __init__(self, groups, num_beams, eos_ids, pad_id, max_new_tokens, length_penalty=1.0, early_stopping=False,
                 num_return_sequences=1):
        if early_stopping not in (False, True, "never"):
            raise ValueError(f"early_stopping={early_stopping!r} must be False, True or 'never'")
        self.G, self.B, self.T = int(groups), int(num_beams), int(max_new_tokens)
        self.eos = torch.tensor(sorted(set(int(e) for e in eos_ids)), dtype=torch.int64)
        self.pad = int(pad_id) if pad_id is not None else (int(eos_ids[0]) if len(eos_ids) else 0)
        self.length_penalty, self.early_stopping, self.n_ret = float(length_penalty), early_stopping, int(num_return_sequences)
        G, B, T = self.G, self.B, self.T
        if B == 1:
            self.early_stopping = True        # greedy search: a prompt ends with its first hypothesis, whatever the heuristic would allow
        self.k =beams_to_keep(B, len(self.eos))
        self.top_mask = torch.arange(self.k) < B
        self.run_seq = torch.full((G, B, T), self.pad, dtype=torch.int64)
        self.run_scores = torch.zeros((G, B), dtype=torch.float32)
        self.run_scores[:, 1:] = DEAD
        self.fin_seq = self.run_seq.clone()
        self.fin_scores = torch.full((G, B), DEAD, dtype=torch.float32)
        self.fin_len = torch.zeros((G, B), dtype=torch.int64)
        self.is_fin = torch.zeros((G, B), dtype=torch.bool)
        self.can_improve = torch.ones((G, 1), dtype=torch.bool)
        self.steps = 0
        self.device = torch.device("cpu")

    def running_scores(self):
        return self.run_scores.reshape(-1).to(self.device)

    @staticmethod
    def _gather(x, idx):
        """x [G, n, ...], idx [G, m] -> x[g, idx[g, j]] as [G, m, ...]"""
        while idx.dim() < x.dim():
            idx = idx.unsqueeze(-1)
        return torch.gather(x, 1, idx.expand(idx.shape[0], idx.shape[1], *x.shape[2:]))

    def step(self, cand_score, cand_beam, cand_token):
        G, B, K, i = self.G, self.B, self.k, self.steps
        if i >= self.T:
            raise RuntimeError("BeamSearch.step: max_new_tokens steps have been taken")
        self.device = cand_score.device
        host = torch.stack([cand_score.double(), cand_beam.double(), cand_token.double()]).cpu()        # the step's one read
        log_probs = host[0].float().reshape(G, K)
        beams, tokens = host[1].long().reshape(G, K).clamp_(min=0), host[2].long().reshape(G, K).clamp_(min=0)

        seqs = self._gather(self.run_seq, beams)
        seqs[:, :, i] = tokens
        hits = torch.isin(tokens, self.eos) | (i + 1 >= self.T)

        # the next running beams: the best num_beams candidates that did not just end
        running = log_probs + hits.to(torch.float32) * DEAD
        nxt = torch.topk(running, k=B)[1]
        self.run_seq, self.run_scores = self._gather(seqs, nxt), self._gather(running, nxt)
        parent = self._gather(beams, nxt) + torch.arange(G).view(-1, 1) * B
        token = self._gather(tokens, nxt)

        # the finished pool: candidates among the first num_beams that just ended, by length-penalised score, against the old pool
        did = hits & self.top_mask[None, :]
        fin = log_probs / ((i + 1) ** self.length_penalty)
        full = torch.all(self.is_fin, dim=-1, keepdim=True) & (self.early_stopping is True)
        fin = fin + full.to(torch.float32) * DEAD
        fin = fin + (~self.can_improve).to(torch.float32) * DEAD
        fin = fin + (~did) * DEAD
        m_scores = torch.cat((self.fin_scores, fin), dim=1)
        keep = torch.topk(m_scores, k=B)[1]
        self.fin_seq = self._gather(torch.cat((self.fin_seq, seqs), dim=1), keep)
        self.fin_len = self._gather(torch.cat((self.fin_len, torch.full((G, K), i + 1, dtype=torch.int64)), dim=1), keep)
        self.is_fin = self._gather(torch.cat((self.is_fin, did), dim=1), keep)
        self.fin_scores = self._gather(m_scores, keep)

        # can a running beam still beat the pool's worst?  (the heuristic of each early_stopping value)
        self.steps = i + 1
        best_len = self.T if (self.early_stopping == "never" and self.length_penalty > 0.0) else self.steps
        best_running = self.run_scores[:, :1] / (best_len ** self.length_penalty)
        worst = torch.where(self.is_fin, torch.min(self.fin_scores, dim=1, keepdim=True)[0], DEAD)
        self.can_improve = self.can_improve & torch.any(best_running > worst, dim=-1, keepdim=True)
        goes_on = torch.any(self.can_improve) & ~(torch.all(self.is_fin) & (self.early_stopping is True)) & ~torch.all(hits)
        return (parent.reshape(-1).to(torch.int32).to(self.device), token.reshape(-1, 1).to(self.device), not bool(goes_on))

    def finalize(self):
        n = self.n_ret
        seqs, lens = self.fin_seq[:, :n].reshape(self.G * n, self.T), self.fin_len[:, :n].reshape(-1)
        new = max(1, int(lens.max())) if self.steps else 0
        return seqs[:, :new].contiguous().to(self.device), self.fin_scores[:, :n].reshape(-1).contiguous().to(self.device)
