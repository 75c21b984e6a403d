"""Linear-chain CRF layer of the `crf` classifier (reference model/crf.py:33-157) on libvbg kernels.

Same parameter (`transitions[i, j]` = score of the transition j -> i, with the START row / STOP column pinned to -10000) and the same
per-document API (`forward(feats, tags)` -> (log Z - gold score) / len, `inference(feats)` -> (path score, tag list)); `nll` /
`decode` take all documents of a batch at once (row ranges `doc_off`), one launch each: forward algorithm + gold score,
backward = (marginals - gold indicators), Viterbi with first-maximum tie breaking like `torch.max`.  `posterior` adds what the
reference's prediction path lacks: the same Viterbi path and score together with log Z and the posterior marginals
p(y_t = i | x) of every row, from one launch (vbg_crf_posterior); `path_logp` the row-by-row log posteriors of a given path, from
which the confidence of any span of it is a sum (vbg_crf_path_logp).  With ops.set_crf_stable(True) / VBG_CRF_STABLE=1 `nll` -- and so
`forward(feats, tags)` -- takes Fn.CrfNllStableFn: the same loss with a gradient whose error does not grow with the document's length.
"""
from collections import namedtuple

import torch
import torch.nn as nn

from vbg import functions as Fn
from vbg import ops

START_TAG = "<START>"
STOP_TAG = "<STOP>"

# path int32 [N], score fp32 [ndoc], logz fp32 [ndoc], marginals fp32 [N, ntag] (rows sum to 1; START / STOP columns are zeros)
CrfPosterior = namedtuple("CrfPosterior", ["path", "score", "logz", "marginals"])


class CRF(nn.Module):
    def __init__(self, tag_to_ix):
        super().__init__()
        self.tag_to_ix = tag_to_ix
        self.tagset_size = len(tag_to_ix)
        assert self.tagset_size <= 64, "the CRF kernels hold one tag per lane of a wave (<= 64 tags)"
        self.transitions = nn.Parameter(torch.randn(self.tagset_size, self.tagset_size))
        self.transitions.data[tag_to_ix[START_TAG], :] = -10000
        self.transitions.data[:, tag_to_ix[STOP_TAG]] = -10000

    def _ends(self):
        return self.tag_to_ix[START_TAG], self.tag_to_ix[STOP_TAG]

    def nll(self, feats: torch.Tensor, tags_i32: torch.Tensor, doc_off: torch.Tensor) -> torch.Tensor:
        """feats [N, T], tags int32 [N], doc_off int32 [ndoc + 1] -> per-document (log Z - gold) / len, shape [ndoc]"""
        s, e = self._ends()
        fn = Fn.CrfNllStableFn if ops.crf_stable_enabled() else Fn.CrfNllFn      # the switch is read at call time (ops.set_crf_stable)
        return fn.apply(feats, self.transitions, tags_i32.contiguous(), doc_off, s, e)

    def decode(self, feats: torch.Tensor, doc_off: torch.Tensor):
        """-> (best tag per row int32 [N], path score per document [ndoc])"""
        s, e = self._ends()
        return ops.crf_viterbi(feats.contiguous(), doc_off, self.transitions.detach().contiguous(), s, e)

    def posterior(self, feats: torch.Tensor, doc_off: torch.Tensor) -> CrfPosterior:
        """`decode`'s path and score, bit for bit, with log Z per document and the marginals of every row: one launch"""
        s, e = self._ends()
        return CrfPosterior(*ops.crf_posterior(feats.detach().contiguous(), doc_off, self.transitions.detach().contiguous(), s, e))

    def path_logp(self, feats: torch.Tensor, doc_off: torch.Tensor, path: torch.Tensor):
        """-> (lm [N], lc [N]): the log marginal of path[t] and its log conditional given path[t-1], row by row (lc of a document's
        first row is its lm): lm[s] + lc[s+1 .. e].sum() = log P(y_s .. y_e = path[s .. e] | x).  path: int32 [N], any tags.  One launch"""
        s, e = self._ends()
        return ops.crf_path_logp(feats.detach().contiguous(), doc_off, self.transitions.detach().contiguous(), s, e, path)

    def forward(self, feats, tags):
        off = torch.tensor([0, feats.shape[0]], dtype=torch.int32).to(feats.device)
        return self.nll(feats, tags.int(), off)

    def inference(self, feats):
        off = torch.tensor([0, feats.shape[0]], dtype=torch.int32).to(feats.device)
        path, score = self.decode(feats.detach(), off)
        return score[0], path.tolist()
