"""CL4SRec (Xie et al., ICDE'22; reference model/sequential/CL4SRec.py): SASRec's encoder and BCE loss plus an InfoNCE term
between the last hidden rows of two augmented views of every sequence (crop, reorder or mask: data/augmentor.py's
SequenceAugmentor).  Config block ``CL4SRec: {n_blocks, drop_rate, n_heads, aug_type, aug_rate, cl_rate}``, ``max.len``.

What runs where:
  * ``engine.views: one`` (default; ``SRH_CL4SREC_VIEWS``) stacks [batch; view 1; view 2] into ONE (3B, L) batch and runs
    the encoder once: padding sits on the right and the mask is causal, so no sequence sees another and the result is the
    three calls' in exact arithmetic.  ``three`` is the reference's three calls, the A/B partner.
  * ``engine.embed: hip`` (default; ``SRH_CL4SREC_EMBED``) takes the embedding front -- both gathers, scale, sum, dropout,
    padding mask -- as one launch (ops.SeqEmbedFn) whose two table gradients, like the BCE's (ops.SeqBceLiveFn), are summed
    over the LIVE rows only in chunks of fixed length (srh_rows_live_sum_f32).  ``torch`` is the front SASRec takes
    (ops.GatherRowsFn twice, mul, add, dropout, mask) and ops.SeqBceFn.  Both fronts are encoder.SeqEncoder.front.
  * ``engine.attention`` as in SASRec; the InfoNCE of the two (B, d) row sets is ops.InfoNceFn (util.loss_torch.InfoNCE for
    a width that entry does not take).  A model on the CPU takes torch's expressions throughout.

The item table has item_num + 2 rows (item_num + 1: the mask token) and is created AFTER the rest of the network, as the
reference replaces it, so ``torch.manual_seed`` reproduces its initial weights and the state_dict order.

Host work of a step: ``StagedViews`` turns the stacked ids and positions, y, neg, the last-row indices of both views and
every plan the routes need into ONE int32 upload (encoder.upload_with_plans), cut into one encoder.Group per pass."""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...data.augmentor import SequenceAugmentor
from ...util.loss_torch import InfoNCE, l2_reg_loss
from ...util.route import route
from ...util.sampler import next_batch_sequence
from .encoder import Group, LastRowScores, upload_with_plans
from .SASRec import SASRec_Model, attention_route


def views_route(conf=None):
    """'one' or 'three': SRH_CL4SREC_VIEWS, else the conf's engine.views, else one stacked encoder pass"""
    return route('SRH_CL4SREC_VIEWS', 'engine.views', conf, ('one', 'three'))


def embed_route(conf=None):
    """'hip' or 'torch': SRH_CL4SREC_EMBED, else the conf's engine.embed, else the kernels"""
    return route('SRH_CL4SREC_EMBED', 'engine.embed', conf)


class StagedViews:
    """One training step on the device.  ``views`` = [(seq, pos, last)] * 3: the batch and its two augmented views, ``last``
    the 1-based position of the row InfoNCE reads (None for the batch).  views='one' makes one group of the stacked
    (3B, L) arrays, 'three' one group per view; embed='hip' builds live plans (ops.live_plan_host), 'torch' the scatter
    plans of ops.GatherRowsFn / ops.SeqBceFn.  Everything travels in one int32 upload.  ``anchor_last`` (DuoRec; None changes
    nothing): the batch's own 1-based last positions -- ``idx`` is then the (3, B) device view [batch; view 1; view 2] of the
    rows to read and ``idx_host`` its host copy."""

    def __init__(self, views, y, neg, device, route_views='one', route_embed='hip', anchor_last=None):
        seqs = [np.asarray(v[0]) for v in views]
        poss = [np.asarray(v[1]) for v in views]
        B, L = seqs[0].shape
        self.B, self.L, self.route_views, self.route_embed = B, L, route_views, route_embed
        seq_all = np.concatenate([s.reshape(-1) for s in seqs])
        pos_all = np.concatenate([p.reshape(-1) for p in poss])
        y, neg = np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1)
        valid = poss[0].reshape(-1) != 0
        per = B * L
        bounds = [(0, len(views) * per)] if route_views == 'one' else [(v * per, (v + 1) * per) for v in range(len(views))]
        # the row of the hidden states each view's InfoNCE reads, as an index into its group's (rows, d) hidden matrix
        lasts = []
        for v in (1, 2):
            base = v * B if route_views == 'one' else 0
            lasts.append((base + np.arange(B)) * L + np.asarray(views[v][2], dtype=np.int64) - 1)
        hip = route_embed == 'hip'
        plans = []
        for lo, hi in bounds:
            s, p = seq_all[lo:hi], pos_all[lo:hi]
            plans += [ops.live_plan_host(s, s != 0), ops.live_plan_host(p, s != 0)] if hip else \
                     [ops.scatter_plan_host(s), ops.scatter_plan_host(p)]
        yn = np.concatenate([y, neg])
        plans.append(ops.live_plan_host(yn, np.concatenate([valid, valid])) if hip else ops.scatter_plan_host(yn))
        head = [seq_all, pos_all, y, neg, lasts[0], lasts[1]]
        if anchor_last is not None:
            # DuoRec: the batch's own last rows (its group's hidden matrix) travel in front of the two views', so the three
            # index vectors lie side by side on the device
            self.idx_host = np.stack([np.arange(B) * L + np.asarray(anchor_last, dtype=np.int64) - 1] + lasts)
            head[4:4] = [self.idx_host[0]]
        cut, dev_plans = upload_with_plans(head, plans, device)
        self.y, self.neg, self.last = cut[2], cut[3], (cut[-2], cut[-1])
        self.idx = cut[4].as_strided((3, B), (B, 1)) if anchor_last is not None else None
        self.groups = [Group(((hi - lo) // L, L), cut[0][lo:hi], cut[1][lo:hi], dev_plans[2 * k:2 * k + 2])
                       for k, (lo, hi) in enumerate(bounds)]
        self.bce_plan = dev_plans[-1]
        self.valid = (cut[1][:per] != 0).to(torch.uint8)
        self.n_valid = int(np.count_nonzero(valid))
        self.live_share = float(np.count_nonzero(seq_all)) / seq_all.size


class CL4SRec(LastRowScores, SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(CL4SRec, self).__init__(conf, training_set, test_set)
        section = self.config['CL4SRec']
        self.aug_type = int(section['aug_type'])
        self.aug_rate = float(section['aug_rate'])
        self.cl_rate = float(section['cl_rate'])
        self.views, self.embed = views_route(conf), embed_route(conf)
        self.model = CL4SRec_Model(self.data, self.emb_size, self.max_len, int(section['n_blocks']),
                                   int(section['n_heads']), float(section['drop_rate']), attention=attention_route(conf))
        self.rec_loss = torch.nn.BCEWithLogitsLoss()
        self.epoch_losses = []

    def augment(self, seq, pos, seq_len):
        """the step's two views, drawn in the reference's order: [(seq, pos, last)] * 2"""
        out = []
        for _ in range(2):
            if self.aug_type == 0:
                out.append(SequenceAugmentor.item_crop(seq, seq_len, self.aug_rate))
            elif self.aug_type == 1:
                out.append((SequenceAugmentor.item_reorder(seq, seq_len, self.aug_rate), pos, seq_len))
            else:
                out.append((SequenceAugmentor.item_mask(seq, seq_len, self.aug_rate, self.data.item_num + 1), pos, seq_len))
        return out

    def train(self):
        net = self.model.cuda()
        adam = torch.optim.Adam(net.parameters(), lr=self.lRate)
        for epoch in range(self.maxEpoch):
            net.train()
            seen = []
            batches = next_batch_sequence(self.data, self.batch_size, max_len=self.max_len)
            for n, (seq, pos, y, neg_idx, seq_len) in enumerate(batches):
                batch_loss, rec_loss, _ = self.step_losses(seq, pos, y, neg_idx, self.augment(seq, pos, seq_len))
                adam.zero_grad()
                batch_loss.backward()
                adam.step()
                seen.append(batch_loss.detach())
                if n % 50 == 0:
                    print('training:', epoch + 1, 'batch', n, 'batch_loss:', batch_loss.item(), 'rec_loss:', rec_loss.item())
            self.epoch_losses.append([float(v) for v in torch.stack(seen).cpu()])
            net.eval()
            self.fast_evaluation(epoch)

    def step_losses(self, seq, pos, y, neg, aug_views):
        """(batch loss, rec loss, cl_rate * InfoNCE) of one batch and its two views ([(seq, pos, last)] * 2)"""
        net = self.model
        dev = net.item_emb.device
        d = self.emb_size
        if dev.type != 'cuda':
            hidden = net.forward(seq, pos)
            rows = []
            for v_seq, v_pos, v_last in aug_views:
                emb = net.forward(v_seq, v_pos)
                last = torch.as_tensor(np.asarray(v_last, dtype=np.int64) - 1)
                rows.append(emb[torch.arange(emb.shape[0]), last])
            rec_loss = self.calculate_loss(hidden, y, neg, pos)
        else:
            staged = StagedViews([(seq, pos, None)] + list(aug_views), y, neg, dev, self.views, self.embed)
            B = staged.B
            if self.views == 'one':
                out = net.forward(None, None, staged=staged, group=0).reshape(-1, d)
                hidden, rows = out[:B * staged.L], [out[staged.last[v].long()] for v in range(2)]
            else:
                hidden = net.forward(None, None, staged=staged, group=0).reshape(-1, d)
                rows = [net.forward(None, None, staged=staged, group=v + 1).reshape(-1, d)[staged.last[v].long()]
                        for v in range(2)]
            rec_loss = self.calculate_loss(hidden, y, neg, pos, staged=staged)
        if rows[0].is_cuda and d in ops.NCE_WIDTHS:
            cl = ops.InfoNceFn.apply(rows[0], rows[1], 1.0)
        else:
            cl = InfoNCE(rows[0], rows[1], 1, True)
        cl_loss = self.cl_rate * cl
        return rec_loss + l2_reg_loss(self.reg, net.item_emb) + cl_loss, rec_loss, cl_loss

    def calculate_loss(self, seq_emb, y, neg, pos, staged=None):
        """both BCE-with-logits means over the positions with pos != 0 (CL4SRec.py:70-79)"""
        table = self.model.item_emb
        hidden = seq_emb.reshape(-1, seq_emb.shape[-1])
        if not hidden.is_cuda:
            idx = torch.from_numpy(np.flatnonzero(np.asarray(pos).reshape(-1) != 0))
            h = hidden[idx]
            yp = torch.from_numpy(np.asarray(y).reshape(-1).astype(np.int64))[idx]
            yn = torch.from_numpy(np.asarray(neg).reshape(-1).astype(np.int64))[idx]
            pos_logits, neg_logits = (h * table[yp]).sum(-1), (h * table[yn]).sum(-1)
            return (self.rec_loss(pos_logits, torch.ones_like(pos_logits))
                    + self.rec_loss(neg_logits, torch.zeros_like(neg_logits)))
        if staged is not None:
            fn = ops.SeqBceLiveFn if staged.route_embed == 'hip' else ops.SeqBceFn
            return fn.apply(hidden, table, staged.y, staged.neg, staged.valid, staged.n_valid, staged.bce_plan)
        dev = hidden.device
        y, neg, valid = np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1), np.asarray(pos).reshape(-1) != 0
        yn = np.concatenate([y, neg])
        ids = torch.from_numpy(np.stack([y, neg, valid]).astype(np.int32)).to(dev)
        if self.embed == 'hip':
            fn, plan = ops.SeqBceLiveFn, ops.live_plan(yn, dev, np.concatenate([valid, valid]))
        else:
            fn, plan = ops.SeqBceFn, ops.scatter_plan(yn, dev)
        return fn.apply(hidden, table, ids[0], ids[1], ids[2].to(torch.uint8), int(np.count_nonzero(valid)), plan)


class CL4SRec_Model(SASRec_Model):
    """SASRec_Model with an item table of item_num + 2 rows (item_num + 1: the mask token)"""

    def _init_model(self):
        super()._init_model()
        # the reference replaces the table once the network stands (CL4SRec.py:23-25): the same draws in the same order
        self.item_rows += 1
        self.item_emb = nn.Parameter(nn.init.xavier_uniform_(torch.empty(self.item_rows, self.emb_size)))
