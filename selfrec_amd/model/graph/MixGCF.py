"""MixGCF (Huang et al., KDD'21; reference model/graph/MixGCF.py:12-129), op-level tier.  Per pair the sampler
draws ``n_negs`` (64) candidates; for every hop the candidates are mixed with the positive (random alpha), the
hardest one by inner product with the user is kept, and the kept ones are averaged over hops.  Config block
``MixGCF: {n_layer, n_negs}``.  The sampler at 64 negatives per pair is this model's hot spot on the host: the C++
replay produces them at tens of millions of draws per second (tools / DESIGN.md).

The mixing itself has two routes, ``engine.mixup`` / ``SRH_MIXGCF_MIXUP``: ``hip`` is ops.MixupFn
(csrc/mixgcf.hip: pick, mix and the row gradients in two kernels, nothing of size B x n_negs x d ever written), ``torch``
the reference's expression (mixup_torch below), its A/B partner in tools/oplevel_probe.py."""
import torch
import torch.nn as nn

from ... import ops
from ...util.loss_torch import bpr_loss, l2_reg_loss
from ...util.route import route
from ._oplevel import OpLevelRecommender, PropagationEncoder

# torch's own rand_like, captured at import from where torch itself binds it: this module may be imported for the first
# time by a caller who has ALREADY replaced torch.rand_like, and that caller is to be obeyed too
_TORCH_RAND_LIKE = getattr(torch._C._VariableFunctions, "rand_like", torch.rand_like)


def mixup_route(conf=None):
    """'hip' (csrc/mixgcf.hip: pick, mix and row gradients in two kernels) or 'torch' (the reference's expression)"""
    return route('SRH_MIXGCF_MIXUP', 'engine.mixup', conf)


def mixup_torch(u, item_hops, pos, neg, n_negs):
    """The reference's hop mixing (MixGCF.py:96-114) on any device: per hop table the candidates are mixed with the
    positive by a ``rand_like`` alpha, the hardest one by inner product with the user row is kept (detached choice), and
    the kept ones are averaged over hops.  -> (the positives' rows of the hop-mean table, the mixed negatives), B x d."""
    d = int(u.shape[1])
    picked = []
    for table in item_hops:
        cand = table[neg].reshape(-1, n_negs, d)
        alpha = torch.rand_like(cand)
        cand = alpha * table[pos].unsqueeze(1) + (1 - alpha) * cand                 # positive mixing
        hardest = (u.unsqueeze(1) * cand).sum(-1).max(dim=1)[1].detach()           # hop-wise hard negative
        picked.append(cand[torch.arange(cand.size(0), device=cand.device), hardest])
    items = torch.stack(list(item_hops), dim=1).mean(dim=1)
    return items[pos], torch.stack(picked, dim=1).mean(dim=1)


class MixGCF_Encoder(PropagationEncoder):
    def __init__(self, data, emb_size, n_negs, n_layers, mixup='torch'):
        super().__init__(data, emb_size, n_layers)
        self.n_negs, self.emb_size = int(n_negs), int(emb_size)
        self.dropout = nn.Dropout(0.1)
        # the kernel route, unless the shape is one the kernels do not serve
        self.mixup = mixup if ops.mixup_supported(self.emb_size, self.n_layers + 1, self.n_negs) else 'torch'
        self.rng_counter = 0          # counter of the next in-kernel alpha draw; advanced by H B C per training forward

    def hop_tables(self):
        """user-side mean over hops and the per-hop item tables, with message dropout after each product
        (MixGCF.py:70-82)"""
        hops = self.hops(between=self.dropout)
        n_u = self.data.user_num
        return torch.stack([h[:n_u] for h in hops], dim=1).mean(dim=1), [h[n_u:] for h in hops]

    def _mixup_hip(self, u, item_hops, pos_item, neg_item):
        """ops.MixupFn over the hop tables as they are.  alpha is drawn in the kernel from (torch.initial_seed(), a counter
        kept here): no draw of any torch generator is consumed.  A caller who replaced torch.rand_like is obeyed: it is
        called once per hop on a (B, n_negs, d) device tensor, in hop order, and its tensors are injected."""
        B, H = int(pos_item.numel()), len(item_hops)
        alpha = None
        if torch.rand_like is not _TORCH_RAND_LIKE:
            like = torch.empty((B, self.n_negs, self.emb_size), dtype=u.dtype, device=u.device)
            alpha = [torch.rand_like(like) for _ in range(H)]
        seed = torch.initial_seed() & ((1 << 63) - 1)
        pos_rows, negs, _pick = ops.MixupFn.apply(u, pos_item, neg_item, self.n_negs, alpha, seed, self.rng_counter,
                                                  *item_hops)
        if self.training:
            self.rng_counter += H * B * self.n_negs
        return pos_rows, negs

    def negative_mixup(self, user, pos_item, neg_item):
        users, item_hops = self.hop_tables()
        u = users[user]
        if self.mixup == 'hip':
            pos_rows, negs = self._mixup_hip(u, item_hops, pos_item, neg_item)
        else:
            pos_rows, negs = mixup_torch(u, item_hops, pos_item, neg_item, self.n_negs)
        return u, pos_rows, negs

    def get_embeddings(self):
        return super().forward()


class MixGCF(OpLevelRecommender):
    def __init__(self, conf, training_set, test_set):
        super().__init__(conf, training_set, test_set)
        block = self.config['MixGCF']
        self.n_layers, self.n_negs = int(block['n_layer']), int(block['n_negs'])
        self.mixup = mixup_route(self.config)
        self.model = MixGCF_Encoder(self.data, self.emb_size, self.n_negs, self.n_layers, self.mixup)

    def batch_loss(self, user_idx, pos_idx, neg_idx):
        u, p, n = self.model.negative_mixup(user_idx, pos_idx, neg_idx)
        return bpr_loss(u, p, n) + l2_reg_loss(self.reg, u, p, n) / self.batch_size

    def snapshot(self):
        self.user_emb, self.item_emb = self.model.get_embeddings()
