"""DuoRec (Qiu et al., WSDM'22, "Contrastive Learning for Representation Degeneration Problem in Sequential Recommendation"):
SASRec's encoder and BCE loss plus two contrastive terms on the last hidden rows of three views of every sequence -- the
batch (view 0), the same ids again, which differ by dropout only (view 1, the unsupervised positive), and a sequence with
the same target item (view 2, the semantic positive: util.sampler.same_target_positives).  The reference ships the conf
(block ``DuoRec: {n_blocks, drop_rate, n_heads, cl_rate}``) and the loss (util/loss_torch.py info_nce, RecBole's) but no
model file; this one follows the reference's CL4SRec wherever DuoRec does not differ:

    loss = rec + l2_reg_loss(reg, item_emb) + cl_rate (info_nce(h_a, h_p, tau, B, sim) + info_nce(h_a, h_q, tau, B, sim))

``rec`` is CL4SRec's two BCE means on view 0, B the true size of a short last batch.  Optional conf keys the reference's
conf lacks: ``tau`` (1.0) and ``sim`` ('dot', or 'cos'), the paper's and RecBole's defaults.  The item table has
item_num + 1 rows (no mask token) and SASRec's creation order.

Routes: ``engine.attention``, ``engine.views`` and ``engine.embed`` as in CL4SRec.  ``engine.duo`` (``SRH_DUOREC_DUO``):
``hip`` reads the three last rows out of the stacked pass's hidden matrix inside ONE fused call for both terms
(ops.DuoNceFn, csrc/duo.hip); ``pair`` is its A/B partner, torch row indexing and two util.loss_torch.info_nce calls.
``sim: cos`` puts ops.RowsL2NormFn in front of either.  A width the kernel does not take goes to ``pair``, announced once.
A model on the CPU takes torch's expressions throughout."""
import warnings

import numpy as np
import torch

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import info_nce, l2_reg_loss
from ...util.route import route
from ...util.sampler import next_batch_sequence_indexed, same_target_positives
from .CL4SRec import CL4SRec, StagedViews, embed_route, views_route
from .encoder import LastRowScores
from .SASRec import SASRec_Model, attention_route

_announced = []


def duo_route(conf=None):
    """'hip' or 'pair': SRH_DUOREC_DUO, else the conf's engine.duo, else the fused kernel"""
    return route('SRH_DUOREC_DUO', 'engine.duo', conf, ('hip', 'pair'))


class DuoRec(LastRowScores, SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(DuoRec, self).__init__(conf, training_set, test_set)
        section = self.config['DuoRec']
        self.cl_rate = float(section['cl_rate'])
        self.tau = float(section['tau']) if 'tau' in section else 1.0
        self.sim = str(section['sim']).strip().lower() if 'sim' in section else 'dot'
        if self.sim not in ('dot', 'cos'):
            raise ValueError(f"DuoRec.sim: {self.sim!r} is neither 'dot' nor 'cos'")
        self.views, self.embed, self.duo = views_route(conf), embed_route(conf), duo_route(conf)
        self.model = SASRec_Model(self.data, self.emb_size, self.max_len, int(section['n_blocks']),
                                  int(section['n_heads']), float(section['drop_rate']), attention=attention_route(conf))
        self.rec_loss = torch.nn.BCEWithLogitsLoss()
        self.epoch_losses = []

    calculate_loss = CL4SRec.calculate_loss

    def train(self):
        net = self.model.cuda()
        adam = torch.optim.Adam(net.parameters(), lr=self.lRate)
        for epoch in range(self.maxEpoch):
            net.train()
            seen = []
            batches = next_batch_sequence_indexed(self.data, self.batch_size, max_len=self.max_len)
            for n, (seq, pos, y, neg_idx, seq_len, rows) in enumerate(batches):
                positives = same_target_positives(self.data, rows, self.max_len)[:3]
                batch_loss, rec_loss, _ = self.step_losses(seq, pos, y, neg_idx, seq_len, positives)
                adam.zero_grad()
                batch_loss.backward()
                adam.step()
                seen.append(batch_loss.detach())
                if n % 50 == 0:
                    print('training:', epoch + 1, 'batch', n, 'batch_loss:', batch_loss.item(), 'rec_loss:', rec_loss.item())
            self.epoch_losses.append([float(v) for v in torch.stack(seen).cpu()])
            net.eval()
            self.fast_evaluation(epoch)

    def duo_kernel(self, on_device=True):
        """whether both contrastive terms run as the one fused call: the route, a model on the device, a width it takes"""
        if self.duo != 'hip' or not on_device:
            return False
        if not ops.duo_supported(self.emb_size):
            if 'width' not in _announced:
                _announced.append('width')
                warnings.warn(f"engine.duo: hip serves rows up to {ops.DUO_WIDTHS[-1]} columns, not {self.emb_size}; "
                              f"taking the pair route", RuntimeWarning, stacklevel=2)
            return False
        return True

    def contrastive(self, h_a, h_p, h_q):
        """cl_rate (info_nce(h_a, h_p) + info_nce(h_a, h_q)) of three (B, d) row sets (the pair route, views 'three', the CPU)"""
        B = int(h_a.shape[0])
        if self.duo_kernel(h_a.is_cuda):
            if self.sim == 'cos':
                h_a, h_p, h_q = ops.RowsL2NormFn.apply(torch.cat((h_a, h_p, h_q))).split(B)
            return ops.DuoNceFn.apply(1.0 / self.tau, self.cl_rate, self.cl_rate, None, None, h_a, h_p, h_q).sum()
        return self.cl_rate * (info_nce(h_a, h_p, self.tau, B, self.sim) + info_nce(h_a, h_q, self.tau, B, self.sim))

    def step_losses(self, seq, pos, y, neg, seq_len, positives):
        """(batch loss, rec loss, the contrastive share) of one batch and its semantic positives (seq, pos, seq_len)"""
        net = self.model
        dev = net.item_emb.device
        d = self.emb_size
        views = [(seq, pos, seq_len), tuple(positives)]
        if dev.type != 'cuda':
            hidden = net.forward(seq, pos)
            rows = [hidden[torch.arange(hidden.shape[0]), torch.as_tensor(np.asarray(seq_len, dtype=np.int64) - 1)]]
            for v_seq, v_pos, v_last in views:
                emb = net.forward(v_seq, v_pos)
                rows.append(emb[torch.arange(emb.shape[0]), torch.as_tensor(np.asarray(v_last, dtype=np.int64) - 1)])
            rec_loss = self.calculate_loss(hidden, y, neg, pos)
            cl_loss = self.contrastive(*rows)
        else:
            staged = StagedViews([(seq, pos, None)] + views, y, neg, dev, self.views, self.embed, anchor_last=seq_len)
            if self.views == 'one':
                out = net.forward(None, None, staged=staged, group=0).reshape(-1, d)
                hidden = out[:staged.B * staged.L]
                if self.duo_kernel() and self.sim == 'dot':
                    cl_loss = ops.DuoNceFn.apply(1.0 / self.tau, self.cl_rate, self.cl_rate, staged.idx, staged.idx_host,
                                                 out).sum()
                else:
                    cl_loss = self.contrastive(*(out[staged.idx[v].long()] for v in range(3)))
            else:
                outs = [net.forward(None, None, staged=staged, group=v).reshape(-1, d) for v in range(3)]
                hidden = outs[0]
                cl_loss = self.contrastive(*(outs[v][staged.idx[v].long()] for v in range(3)))
            rec_loss = self.calculate_loss(hidden, y, neg, pos, staged=staged)
        return rec_loss + l2_reg_loss(self.reg, net.item_emb) + cl_loss, rec_loss, cl_loss
