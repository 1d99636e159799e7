"""GRU4Rec (Hidasi et al., ICLR'16) as the sequential family's recurrent baseline: an item embedding followed by a GRU,
trained as SASRec is -- next_batch_sequence, one sampled negative per position, the two BCE means over the positions with
pos != 0, l2_reg_loss on the item table.  The reference ships no GRU4Rec.py; DESIGN.md 4.30 is the model's specification,
and it follows the reference's SASRec wherever a GRU does not differ.  Config block ``GRU4Rec: {n_layers, drop_rate}``.

    x   = emb_dropout(item_emb[seq]) * live          (no position table, no scale by sqrt(d))
    h_t = GRU(x), t = 0 .. len_b - 1, h_{-1} = 0     (torch.nn.GRU: gate order r, z, n, both biases, torch's init)
    out = h * live                                   (exact zeros at the padding, which sits on the right)

What runs where: ``engine.rnn: hip`` (``SRH_GRU4REC_RNN``) runs every layer as ops.GruFn -- F.linear for the
input side, ONE launch each way for the recurrence (csrc/gru.hip), which stops at every sequence's own length.
``engine.rnn: torch`` is nn.GRU's own forward over all max.len steps times ``live``: the A/B partner, the route of a shape
outside the kernels' envelope and of a model on the CPU.  The item gather's gradient walks the live rows only
(ops.GatherLiveRowsFn), as the loss's does (ops.SeqBceLiveFn); ``StagedSeqBatch`` uploads a step's ids, lengths and both
plans in one copy.  Evaluation and prediction are the base class's over LastRowScores."""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import l2_reg_loss
from ...util.route import route
from ...util.sampler import next_batch_sequence
from .encoder import LastRowScores, upload_with_plans

RNN_DEFAULT = 'torch'


def rnn_route(conf=None):
    """'hip' or 'torch': SRH_GRU4REC_RNN, else the conf's engine.rnn, else RNN_DEFAULT (DESIGN.md 4.30 has the A/B)"""
    choices = ('hip', 'torch') if RNN_DEFAULT == 'hip' else ('torch', 'hip')
    return route('SRH_GRU4REC_RNN', 'engine.rnn', conf, choices)


class StagedSeqBatch:
    """One (B, L) batch on the device: the item ids, the sequence lengths, and for a training batch the targets, the
    negatives and the live plans of the item gather (``item_plan``) and of [y; neg] (``bce_plan``), all in ONE int32
    upload.  item_plan=False (evaluation: no gradient reaches the table) uploads ids and lengths only."""

    def __init__(self, seq, device, pos=None, y=None, neg=None, item_plan=True):
        seq = np.asarray(seq)
        self.shape = tuple(seq.shape)
        flat = seq.reshape(-1)
        ids, plans = [flat, np.count_nonzero(seq, axis=1)], []
        if item_plan:
            plans.append(ops.live_plan_host(flat))
        if y is not None:
            valid = np.asarray(pos).reshape(-1) != 0
            y, neg = np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1)
            ids += [y, neg, valid]
            plans.append(ops.live_plan_host(np.concatenate([y, neg]), np.concatenate([valid, valid])))
            self.n_valid = int(np.count_nonzero(valid))
        views, plans = upload_with_plans(ids, plans, device)
        self.item_plan = plans.pop(0) if item_plan else None
        self.bce_plan = plans.pop(0) if y is not None else None
        self.seq, self.lens = views[0], views[1]
        self.live = (self.seq != 0).reshape(*self.shape, 1)
        self.y, self.neg, valid = views[2:5] if y is not None else (None, None, None)
        self.valid = None if valid is None else valid.to(torch.uint8)


class GRU4Rec_Model(nn.Module):
    """item_num + 1 item rows (0: padding) and an n_layers GRU of width emb_size; created in this order, so
    ``torch.manual_seed`` fixes the initial weights"""

    def __init__(self, data, emb_size, n_layers, drop_rate, rnn=RNN_DEFAULT):
        super(GRU4Rec_Model, self).__init__()
        self.emb_size, self.n_layers, self.drop_rate, self.rnn = emb_size, n_layers, drop_rate, rnn
        self.item_emb = nn.Parameter(nn.init.xavier_uniform_(torch.empty(data.item_num + 1, emb_size)))
        self.emb_dropout = nn.Dropout(drop_rate)
        self.gru = nn.GRU(emb_size, emb_size, num_layers=n_layers, batch_first=True)

    def uses_kernel(self, L, on_device=True):
        """whether the recurrence over L positions runs on the fused kernels: the route, the envelope, and a model that
        lives on the device"""
        return self.rnn == 'hip' and bool(on_device) and ops.gru_supported(int(L), self.emb_size)

    def recurrence(self, x, live, lens):
        """(B, L, d) hidden states of the (B, L, d) inputs, exact zeros where live is False"""
        if self.uses_kernel(x.shape[1], x.is_cuda):
            for layer in range(self.n_layers):
                w_ih, w_hh, b_ih, b_hh = (getattr(self.gru, f'{name}_l{layer}')
                                          for name in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
                x = ops.GruFn.apply(x, w_ih, w_hh, b_ih, b_hh, lens)
            return x
        return self.gru(x)[0] * live

    def forward(self, seq, pos, staged=None):
        """(B, L, d) hidden states of the id array seq (0 = padding, on the right), or of a batch already on the device
        (StagedSeqBatch).  pos: SeqEncoder.forward's argument, not read (the model has no position table)."""
        dev = self.item_emb.device
        live_rows = torch.is_grad_enabled() and ops.seq_embed_supported(self.emb_size)
        if staged is None and dev.type == 'cuda':
            staged = StagedSeqBatch(seq, dev, item_plan=live_rows)
        if staged is not None:
            if live_rows and staged.item_plan is not None:
                items = ops.GatherLiveRowsFn.apply(self.item_emb, staged.seq, staged.item_plan)
            else:
                items = self.item_emb[staged.seq.long()]
            x = self.emb_dropout(items.reshape(*staged.shape, self.emb_size)) * staged.live
            return self.recurrence(x, staged.live, staged.lens)
        ids = torch.from_numpy(np.asarray(seq).astype(np.int64)).to(dev)
        live = (ids != 0).unsqueeze(-1)
        return self.recurrence(self.emb_dropout(self.item_emb[ids]) * live, live, None)


class GRU4Rec(LastRowScores, SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(GRU4Rec, self).__init__(conf, training_set, test_set)
        section = self.config['GRU4Rec']
        self.model = GRU4Rec_Model(self.data, self.emb_size, int(section['n_layers']), float(section['drop_rate']),
                                   rnn=rnn_route(conf))
        self.rec_loss = torch.nn.BCEWithLogitsLoss()
        self.epoch_losses = []

    def train(self):
        net = self.model.cuda()
        adam = torch.optim.Adam(net.parameters(), lr=self.lRate)
        device = net.item_emb.device
        for epoch in range(self.maxEpoch):
            net.train()
            seen = []
            batches = next_batch_sequence(self.data, self.batch_size, max_len=self.max_len)
            for n, (seq, pos, y, neg_idx, _lens) in enumerate(batches):
                staged = StagedSeqBatch(seq, device, pos, y, neg_idx)
                hidden = net.forward(seq, pos, staged=staged)
                batch_loss = self.calculate_loss(hidden, y, neg_idx, pos, staged=staged) + l2_reg_loss(self.reg, net.item_emb)
                adam.zero_grad()
                batch_loss.backward()
                adam.step()
                seen.append(batch_loss.detach())
                if n % 50 == 0:
                    print('training:', epoch + 1, 'batch', n, 'rec_loss:', batch_loss.item())
            self.epoch_losses.append([float(v) for v in torch.stack(seen).cpu()])
            net.eval()
            self.fast_evaluation(epoch)

    def calculate_loss(self, seq_emb, y, neg, pos, staged=None):
        """both BCE-with-logits means over the positions with pos != 0 (reference SASRec.py:44-53): one kernel on the
        device, torch's expression for a model on the CPU"""
        table = self.model.item_emb
        hidden = seq_emb.reshape(-1, seq_emb.shape[-1])
        if not hidden.is_cuda:
            idx = torch.from_numpy(np.flatnonzero(np.asarray(pos).reshape(-1) != 0))
            yp = torch.from_numpy(np.asarray(y).reshape(-1).astype(np.int64))[idx]
            yn = torch.from_numpy(np.asarray(neg).reshape(-1).astype(np.int64))[idx]
            h = hidden[idx]
            pos_logits, neg_logits = (h * table[yp]).sum(-1), (h * table[yn]).sum(-1)
            return (self.rec_loss(pos_logits, torch.ones_like(pos_logits))
                    + self.rec_loss(neg_logits, torch.zeros_like(neg_logits)))
        if staged is not None and staged.y is not None:
            return ops.SeqBceLiveFn.apply(hidden, table, staged.y, staged.neg, staged.valid, staged.n_valid, staged.bce_plan)
        y, neg, valid = np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1), np.asarray(pos).reshape(-1) != 0
        ids = torch.from_numpy(np.stack([y, neg, valid]).astype(np.int32)).to(hidden.device)
        plan = ops.live_plan(np.concatenate([y, neg]), hidden.device, np.concatenate([valid, valid]))
        return ops.SeqBceLiveFn.apply(hidden, table, ids[0], ids[1], ids[2].to(torch.uint8), int(np.count_nonzero(valid)), plan)
