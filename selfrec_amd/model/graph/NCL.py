"""NCL (Lin et al., WWW'22; reference model/graph/NCL.py:11-133), op-level tier: LightGCN propagation on the HIP SpMM,
the structure-contrastive loss of the batch rows against the whole user and item tables on the table InfoNCE kernel
(``ssl_layer_loss``), the prototype loss on the fused InfoNCE, and the E-step's k-means on the device (ops.kmeans, in
place of faiss).  Config block ``NCL: {n_layer, ssl_reg, proto_reg, tau, hyper_layers, alpha, num_clusters}``."""
import numpy as np
import torch

from ... import ops
from ...util.loss_torch import InfoNCE, bpr_loss, l2_reg_loss
from ._oplevel import OpLevelRecommender, PropagationEncoder


class _TableNceFn(torch.autograd.Function):
    """ssl_reg * (L_user + alpha * L_item) of NCL.py:57-83: both sides in one call of the table kernel, which produces
    the loss and both gradients at once; backward() scales them by the upstream gradient."""

    @staticmethod
    def forward(ctx, q_user, t_user, q_item, t_item, user_idx, item_idx, tau, scale_user, scale_item):
        (lu, gqu, gtu), (li, gqi, gti) = ops.table_nce_fwd_bwd(
            [(q_user, t_user, user_idx, scale_user), (q_item, t_item, item_idx, scale_item)], tau=tau)
        ctx.save_for_backward(gqu, gtu, gqi, gti)
        return (lu + li).to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        gqu, gtu, gqi, gti = ctx.saved_tensors
        return gqu * gout, gtu * gout, gqi * gout, gti * gout, None, None, None, None, None


class NCL(OpLevelRecommender):
    warm_up_epochs = 20      # NCL.py:90,104: the prototype loss (and the E-step) from epoch 20 on

    def __init__(self, conf, training_set, test_set):
        super().__init__(conf, training_set, test_set)
        args = self.config['NCL']
        self.n_layers = int(args['n_layer'])
        self.ssl_temp = float(args['tau'])
        self.ssl_reg = float(args['ssl_reg'])
        self.hyper_layers = int(args['hyper_layers'])
        self.alpha = float(args['alpha'])
        self.proto_reg = float(args['proto_reg'])
        self.k = int(args['num_clusters'])
        if self.n_layers < 2 * self.hyper_layers:
            raise ValueError(f"NCL: n_layer = {self.n_layers} < 2 * hyper_layers = {2 * self.hyper_layers}: the context "
                             f"layer hyper_layers * 2 does not exist (the reference fails here with an IndexError)")
        self.model = PropagationEncoder(self.data, self.emb_size, self.n_layers)
        self.user_centroids = None
        self.user_2cluster = None
        self.item_centroids = None
        self.item_2cluster = None

    def e_step(self):
        user_embeddings = self.model.embedding_dict['user_emb'].detach()
        item_embeddings = self.model.embedding_dict['item_emb'].detach()
        self.user_centroids, self.user_2cluster = self.run_kmeans(user_embeddings)
        self.item_centroids, self.item_2cluster = self.run_kmeans(item_embeddings)

    def run_kmeans(self, x):
        """(centroids (k, d), node -> cluster (n,) int64) on the device: ops.kmeans, faiss.Kmeans(d, k)'s defaults"""
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(x).cuda()
        return ops.kmeans(x.float().contiguous(), self.k)

    def ProtoNCE_loss(self, initial_emb, user_idx, item_idx):
        user_emb, item_emb = torch.split(initial_emb, [self.data.user_num, self.data.item_num])
        user2cluster = self.user_2cluster[user_idx]
        user2centroids = self.user_centroids[user2cluster]
        proto_nce_loss_user = InfoNCE(user_emb[user_idx], user2centroids, self.ssl_temp) * self.batch_size
        item2cluster = self.item_2cluster[item_idx]
        item2centroids = self.item_centroids[item2cluster]
        proto_nce_loss_item = InfoNCE(item_emb[item_idx], item2centroids, self.ssl_temp) * self.batch_size
        proto_nce_loss = self.proto_reg * (proto_nce_loss_user + proto_nce_loss_item)
        return proto_nce_loss

    def ssl_layer_loss(self, context_emb, initial_emb, user, item):
        context_user_emb_all, context_item_emb_all = torch.split(context_emb, [self.data.user_num, self.data.item_num])
        initial_user_emb_all, initial_item_emb_all = torch.split(initial_emb, [self.data.user_num, self.data.item_num])
        user, item = torch.as_tensor(user, device=context_emb.device), torch.as_tensor(item, device=context_emb.device)
        return _TableNceFn.apply(context_user_emb_all[user], initial_user_emb_all, context_item_emb_all[item],
                                 initial_item_emb_all, user, item, self.ssl_temp, self.ssl_reg, self.ssl_reg * self.alpha)

    def forward_all(self):
        """(user rows, item rows, [E0, A E0, ...]): LGCN_Encoder.forward (NCL.py:152-162)"""
        emb_list = self.model.hops()
        mean = torch.stack(emb_list, dim=1).mean(dim=1)
        return mean[:self.data.user_num], mean[self.data.user_num:], emb_list

    def batch_losses(self, user_idx, pos_idx, neg_idx, proto):
        """the step's loss terms in NCL.py:93-111's order: (rec, ssl, proto or None, total)"""
        rec_user_emb, rec_item_emb, emb_list = self.forward_all()
        user_emb, pos_item_emb, neg_item_emb = rec_user_emb[user_idx], rec_item_emb[pos_idx], rec_item_emb[neg_idx]
        rec_loss = bpr_loss(user_emb, pos_item_emb, neg_item_emb)
        initial_emb = emb_list[0]
        context_emb = emb_list[self.hyper_layers * 2]
        ssl_loss = self.ssl_layer_loss(context_emb, initial_emb, user_idx, pos_idx)
        total = rec_loss + l2_reg_loss(self.reg, user_emb, pos_item_emb, neg_item_emb) / self.batch_size + ssl_loss
        proto_loss = None
        if proto:
            proto_loss = self.ProtoNCE_loss(initial_emb, user_idx, pos_idx)
            total = total + proto_loss
        return rec_loss, ssl_loss, proto_loss, total

    def train(self):
        from ...util.sampler import next_batch_pairwise
        model = self.model.cuda()
        optimizer = torch.optim.Adam(model.parameters(), lr=self.lRate)
        for epoch in range(self.maxEpoch):
            proto = epoch >= self.warm_up_epochs
            if proto:
                self.e_step()
            for n, batch in enumerate(next_batch_pairwise(self.data, self.batch_size, as_arrays=True)):
                user_idx, pos_idx, neg_idx = (torch.from_numpy(a).cuda() for a in batch)
                model.train()
                rec_loss, ssl_loss, proto_loss, loss = self.batch_losses(user_idx, pos_idx, neg_idx, proto)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                if n % 100 == 0 and n > 0:
                    if proto:
                        print('training:', epoch + 1, 'batch', n, 'rec_loss:', rec_loss.item(), 'ssl_loss', ssl_loss.item(),
                              'proto_loss', proto_loss.item())
                    else:
                        print('training:', epoch + 1, 'batch', n, 'rec_loss:', rec_loss.item(), 'ssl_loss', ssl_loss.item())
            model.eval()
            with torch.no_grad():
                self.snapshot()
            self.fast_evaluation(epoch)
        self.restore_best()

    def snapshot(self):
        self.user_emb, self.item_emb = self.model()
