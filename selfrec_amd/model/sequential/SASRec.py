"""SASRec (Kang & McAuley, ICDM'18; reference model/sequential/SASRec.py): a causal transformer over each item sequence,
trained with one sampled negative per position.  Config block ``SASRec: {n_blocks, drop_rate, n_heads}``, ``max.len``.

What runs where: the attention core of every block -- scores, causal mask, softmax, dropout on the
probabilities, the product with V -- is one fused launch each way (ops.SeqAttnFn, csrc/seqrec.hip), and the loss with
its gradients is one kernel (ops.SeqBceFn); the gathers of the item and position tables scatter their gradients in a
fixed order (ops.GatherRowsFn).  LayerNorm, the Linear layers and Adam are torch's.  ``engine.attention: torch`` (or
``SRH_SASREC_ATTN=torch``) routes the attention core through torch's own expression on the same projected inputs: the A/B
partner of the kernel, and the route of shapes outside its envelope (``max.len`` > 64).

The network is encoder.SeqEncoder, shared with BERT4Rec and CL4SRec (its docstring has the block's semantics): here with
item_num + 1 and max_len + 1 table rows, ReLU and only a causal mask (padding sits on the right, so no valid row sees it).

Host work of a step: ``StagedBatch`` turns the sampler's four id arrays into ONE int32 upload that also
carries the three scatter plans (items, positions, [targets; negatives]); forward and loss read views of it."""
import numpy as np
import torch

from ... import ops
from ...base.seq_recommender import SequentialRecommender
from ...util.loss_torch import l2_reg_loss
from ...util.route import route
from ...util.sampler import next_batch_sequence
from .encoder import LastRowScores, SeqEncoder, StagedIds
from .encoder import torch_causal_attention  # noqa: F401  (a public name of this module: tests and probes import it here)


def attention_route(conf=None):
    """'hip', 'torch' or 'tiled': SRH_SASREC_ATTN, else the conf's engine.attention, else the kernel.  'tiled' is 'hip' plus
    the tiled kernels for 64 < max.len <= 512, which 'hip' leaves to torch's expression"""
    return route('SRH_SASREC_ATTN', 'engine.attention', conf, ('hip', 'torch', 'tiled'))


class StagedBatch(StagedIds):
    """One training batch on the device: ids, masks and the scatter plans of its three gathers, uploaded together."""

    def __init__(self, seq, pos, y, neg, device):
        targets = [] if y is None else [np.asarray(y).reshape(-1), np.asarray(neg).reshape(-1)]
        super().__init__(seq, pos, device, targets, [ops.scatter_plan_host(np.concatenate(targets))] if targets else [])
        self.y, self.neg = self.extra
        self.valid = (self.pos != 0).to(torch.uint8)
        self.n_valid = int(np.count_nonzero(pos))


class SASRec(LastRowScores, SequentialRecommender):
    def __init__(self, conf, training_set, test_set):
        super(SASRec, self).__init__(conf, training_set, test_set)
        section = self.config['SASRec']
        self.model = SASRec_Model(self.data, self.emb_size, self.max_len, int(section['n_blocks']),
                                  int(section['n_heads']), float(section['drop_rate']), attention=attention_route(conf))
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
                staged = StagedBatch(seq, pos, y, neg_idx, device)
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
        """both BCE-with-logits means over the positions with pos != 0 (SASRec.py:44-53), one kernel"""
        if staged is None or staged.y is None:
            staged = StagedBatch(pos, pos, y, neg, seq_emb.device)
        hidden = seq_emb.reshape(-1, seq_emb.shape[-1])
        return ops.SeqBceFn.apply(hidden, self.model.item_emb, staged.y, staged.neg, staged.valid, staged.n_valid,
                                  staged.plans[2])


class SASRec_Model(SeqEncoder):
    """the causal encoder: item_num + 1 item rows (0: padding), max_len + 1 positions, ReLU"""

    def __init__(self, data, emb_size, max_len, n_blocks, n_heads, drop_rate, attention='hip'):
        super(SASRec_Model, self).__init__(data.item_num + 1, max_len + 1, emb_size, n_blocks, n_heads, drop_rate, attention)
