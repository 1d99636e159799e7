"""SEPT (Yu et al., KDD'21; reference model/graph/SEPT.py:17-198, a TF1 graph there), op-level tier: socially-aware
tri-training.  Config block ``SEPT: {n_layer, ss_rate, drop_rate, ins_cnt}`` and the ``social.data`` file.

Four encoders share the two embedding tables: ``rec`` propagates [users; items] over the normalised adjacency, ``aug``
over the epoch's edge-dropped Laplacian, ``friend`` and ``sharing`` propagate the USER table over the two social views
(``get_social_related_views``, host scipy, the reference's arithmetic).  Every layer is l2_normalize(A x) and an encoder's
output is the SUM of the raw table and its normalised layers (SEPT.py:48-64).  Each encoder labels, for every unique user
of a batch, the ``ins_cnt`` users the OTHER two encoders find closest in the aug view (softmax of cosine scores, averaged,
top-k), and is trained to tell them from the rest of the batch (neighbor_discrimination, temperature 0.1).

What runs where:
  * propagation: the HIP SpMM; with the row normalise behind it, forward and backward, ``ops.NormPropFn``
    (``engine.norm: torch`` / ``SRH_SEPT_NORM``: torch's rsqrt / clamp expression around the same SpMM);
  * label_prediction -> top_k -> neighbor_discrimination: ``ops.TriNdFn`` (csrc/sept.hip), no n x n matrix in memory
    (``engine.nd: torch`` / ``SRH_SEPT_ND``: the reference's expression on materialised matrices, same device);
  * bpr_loss of util/loss_tf.py (-sum log(sigmoid(x) + 10e-8), a SUM) and the whole-table regulariser
    reg * (sum U^2 / 2 + sum I^2 / 2): element-wise torch, as the reference writes them;
  * training as the reference schedules it: rec-only epochs while ``epoch <= maxEpoch / 3`` under one Adam, joint epochs
    after that under a SECOND Adam with its own moments and step count; the dropped adjacency is redrawn once per joint
    epoch (GraphAugmentor.edge_dropout, the reference's keep-set on the global ``random`` stream); evaluation and save()
    use the ``rec`` embeddings.

Stated deviations from the reference: ``torch.optim.Adam`` adds eps to sqrt(v_hat) where TF1's AdamOptimizer adds it to
sqrt(v) before the bias correction; the initial tables come from torch's RNG (xavier_uniform_), not TF's."""
import numpy as np
import torch
import torch.nn as nn
from scipy.sparse import eye

from ... import ops
from ...base.torch_interface import TorchGraphInterface
from ...data.augmentor import GraphAugmentor
from ...data.social import Relation
from ...util.route import route
from ._oplevel import OpLevelRecommender

TAU = 0.1                             # SEPT.py:131-132
PAIRS = ((1, 2), (0, 2), (0, 1))      # SEPT.py:145-147: the two views that label friend / sharing / rec


def nd_route(conf=None):
    """'hip' or 'torch': SRH_SEPT_ND, else the conf's engine.nd, else the kernels"""
    return route('SRH_SEPT_ND', 'engine.nd', conf)


def norm_route(conf=None):
    """'hip' or 'torch': SRH_SEPT_NORM, else the conf's engine.norm, else the kernels"""
    return route('SRH_SEPT_NORM', 'engine.norm', conf)


def l2_normalize(x):
    """tf.math.l2_normalize(x, axis=1) in torch: x * rsqrt(max(sum x^2, 1e-12))"""
    return x * torch.rsqrt(torch.clamp((x * x).sum(dim=1, keepdim=True), min=1e-12))


def tf_bpr_loss(user_emb, pos_item_emb, neg_item_emb):
    """util/loss_tf.py:4-7"""
    score = (user_emb * pos_item_emb).sum(dim=1) - (user_emb * neg_item_emb).sum(dim=1)
    return -torch.log(torch.sigmoid(score) + 10e-8).sum()


def tri_nd_torch(friend, sharing, rec, aug, k, tau=TAU, pos=None):
    """SEPT.py:98-134 as the reference writes it, on materialised n x n matrices -> (summed loss, pos (3, n, k)).
    ``pos`` given: the loss of those positives instead of the top-k's."""
    a = l2_normalize(aug)
    scores = [l2_normalize(v) @ a.T for v in (friend, sharing, rec)]
    if pos is None:
        prob = [torch.softmax(s, dim=1) for s in scores]
        pos = torch.stack([torch.topk((prob[p] + prob[q]) / 2, k, dim=1)[1] for p, q in PAIRS])
    loss = 0
    for v, s in enumerate(scores):
        pos_score = torch.exp(torch.gather(s, 1, pos[v].long()) / tau).sum(dim=1)
        ttl_score = torch.exp(s / tau).sum(dim=1)
        loss = loss - torch.log(pos_score / ttl_score).sum()
    return loss, pos


def social_related_views(social_data, social_mat, interaction_mat):
    """SEPT.py:33-40: [friend view, sharing view] -- friends who are friends of friends, friends who share an item, each
    plus the identity, symmetrically normalised.  Host scipy in float32, the reference's arithmetic."""
    identity = eye(social_mat.shape[0], dtype=np.float32)
    social_matrix = social_mat.dot(social_mat).multiply(social_mat) + identity
    sharing_matrix = interaction_mat.dot(interaction_mat.T).multiply(social_mat) + identity
    return [social_data.normalize_graph_mat(social_matrix), social_data.normalize_graph_mat(sharing_matrix)]


class SEPT_Encoder(nn.Module):
    """The two tables (users first, then items: the reference's creation order) and the four adjacencies."""

    def __init__(self, data, emb_size, n_layers, friend_mat, sharing_mat, norm='hip'):
        super().__init__()
        self.data, self.n_layers, self.norm = data, int(n_layers), norm
        make = lambda rows: nn.Parameter(nn.init.xavier_uniform_(torch.empty(rows, emb_size)))  # noqa: E731
        self.embedding_dict = nn.ParameterDict({"user_emb": make(data.user_num), "item_emb": make(data.item_num)})
        convert = TorchGraphInterface.convert_sparse_mat_to_tensor
        self.sparse_norm_adj = convert(data.norm_adj).cuda()
        self.friend_adj = convert(friend_mat).cuda()
        self.sharing_adj = convert(sharing_mat).cuda()

    def layer(self, adj, x):
        if self.norm == 'hip':
            return ops.NormPropFn.apply(adj, x)
        return l2_normalize(torch.sparse.mm(adj, x))

    def encode(self, emb, adj):
        total = emb
        for _ in range(self.n_layers):
            emb = self.layer(adj, emb)
            total = total + emb
        return total

    def forward(self, adj=None):
        """SEPT.encoder: (user rows, item rows) over the normalised adjacency, or over ``adj``"""
        table = torch.cat([self.embedding_dict["user_emb"], self.embedding_dict["item_emb"]], 0)
        out = self.encode(table, self.sparse_norm_adj if adj is None else adj)
        return out[:self.data.user_num], out[self.data.user_num:]

    def social(self, adj):
        """SEPT.social_encoder: the user table over a social view"""
        return self.encode(self.embedding_dict["user_emb"], adj)


class SEPT(OpLevelRecommender):
    def __init__(self, conf, training_set, test_set, **kwargs):
        super().__init__(conf, training_set, test_set, **kwargs)
        args = self.config['SEPT']
        self.n_layers = int(args['n_layer'])
        self.ss_rate = float(args['ss_rate'])
        self.drop_rate = float(args['drop_rate'])
        self.instance_cnt = int(args['ins_cnt'])
        if not 1 <= self.instance_cnt <= ops.TRI_ND_MAX_K and nd_route(conf) == 'hip':
            raise ValueError(f"SEPT: ins_cnt = {self.instance_cnt}: the kernel keeps 1 .. {ops.TRI_ND_MAX_K} positives per "
                             f"row (engine.nd: torch serves any)")
        self.social_data = Relation(conf, kwargs['social.data'], self.data.user)
        self.nd, self.norm = nd_route(conf), norm_route(conf)
        self.bi_social_mat = self.social_data.get_birectional_social_mat()
        self.social_mat, self.sharing_mat = self.get_social_related_views(self.bi_social_mat, self.data.interaction_mat)
        self.model = SEPT_Encoder(self.data, self.emb_size, self.n_layers, self.social_mat, self.sharing_mat, self.norm)
        self.sub_mat = self.dropped = None
        self.optimizers = None
        self.last_pos = None

    def print_model_info(self):
        super().print_model_info()
        print('Social data size: (user number: %d, relation number: %d).' % (self.social_data.size()))
        print('=' * 80)

    def get_social_related_views(self, social_mat, interaction_mat):
        return social_related_views(self.social_data, social_mat, interaction_mat)

    def redraw(self):
        """a joint epoch's edge-dropped Laplacian (SEPT.py:165-168)"""
        self.dropped = GraphAugmentor.edge_dropout(self.data.interaction_mat, self.drop_rate)
        self.sub_mat = TorchGraphInterface.convert_sparse_mat_to_tensor(self.data.convert_to_laplacian_mat(self.dropped)).cuda()

    def neighbor_dis_loss(self, friend, sharing, rec, aug, pos=None):
        """the three neighbor_discrimination losses summed, on the (n x d) rows of the batch's unique users"""
        n = int(aug.shape[0])
        if n < self.instance_cnt:
            raise ValueError(f"SEPT: a batch with {n} unique users cannot give ins_cnt = {self.instance_cnt} positives per "
                             f"user; lower ins_cnt or raise batch.size (the reference's top_k fails here as well)")
        if self.nd == 'hip' and pos is None:
            loss = ops.TriNdFn.apply(friend, sharing, rec, aug, self.instance_cnt, TAU)
            self.last_pos = ops.TriNdFn.last_pos
            return loss
        loss, self.last_pos = tri_nd_torch(friend, sharing, rec, aug, self.instance_cnt, TAU, pos)
        return loss

    def batch_losses(self, user_idx, pos_idx, neg_idx, joint, pos=None, uniq=None):
        """(rec_loss, neighbor_dis_loss or None, the loss its optimiser minimises) of one batch, SEPT.py:138-154"""
        model = self.model
        rec_user_emb, rec_item_emb = model()
        table = model.embedding_dict
        rec_loss = tf_bpr_loss(rec_user_emb[user_idx], rec_item_emb[pos_idx], rec_item_emb[neg_idx])
        rec_loss = rec_loss + self.reg * ((table["user_emb"] ** 2).sum() / 2 + (table["item_emb"] ** 2).sum() / 2)
        if not joint:
            return rec_loss, None, rec_loss
        if self.sub_mat is None:
            self.redraw()
        aug_user_emb, _ = model(self.sub_mat)
        sharing_view = model.social(model.sharing_adj)
        friend_view = model.social(model.friend_adj)
        if uniq is None:     # tf.unique keeps first-occurrence order (train() computes it from the host batch instead)
            uniq = torch.from_numpy(ops.unique_first(user_idx.cpu().numpy())).to(user_idx.device)
        nd_loss = self.neighbor_dis_loss(friend_view[uniq], sharing_view[uniq], rec_user_emb[uniq], aug_user_emb[uniq], pos)
        return rec_loss, nd_loss, rec_loss + self.ss_rate * nd_loss

    def is_joint(self, epoch):
        return epoch > self.maxEpoch / 3      # SEPT.py:163 (float division)

    def train(self):
        from ...util.sampler import next_batch_pairwise
        model = self.model.cuda()
        params = list(model.parameters())
        # SEPT.py:155-158: v1_opt minimises rec_loss, v2_opt the joint loss; each keeps its own moments and step count
        self.optimizers = {'rec': torch.optim.Adam(params, lr=self.lRate), 'joint': torch.optim.Adam(params, lr=self.lRate)}
        for epoch in range(self.maxEpoch):
            joint = self.is_joint(epoch)
            if joint:
                self.redraw()
            optimizer = self.optimizers['joint' if joint else 'rec']
            model.train()
            for n, batch in enumerate(next_batch_pairwise(self.data, self.batch_size, as_arrays=True)):
                user_idx, pos_idx, neg_idx = (torch.from_numpy(a).cuda() for a in batch)
                # the unique users in first-occurrence order, from the host ids: one upload per step, no read-back
                uniq = torch.from_numpy(ops.unique_first(batch[0])).cuda() if joint else None
                rec_loss, nd_loss, loss = self.batch_losses(user_idx, pos_idx, neg_idx, joint, uniq=uniq)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                if n % self.verbose_every == 0 and n > 0:
                    if joint:
                        print('training:', epoch + 1, 'batch', n, 'rec loss:', rec_loss.item(), 'con_loss:',
                              self.ss_rate * nd_loss.item())
                    else:
                        print('training:', epoch + 1, 'batch', n, 'rec loss:', rec_loss.item())
            model.eval()
            with torch.no_grad():
                self.snapshot()
            self.fast_evaluation(epoch)
        self.restore_best()

    def snapshot(self):
        self.user_emb, self.item_emb = self.model()
