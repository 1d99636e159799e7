"""SSL4Rec (Yao et al., CIKM'21; reference model/graph/SSL4Rec.py): two-tower retrieval with in-batch softmax and a
feature-dropout contrastive loss on the item tower.  Config block ``SSL4Rec: {tau, alpha, drop}``.

Every step runs on csrc/ssl4rec.hip: the towers (Linear(64, 1024) -> ReLU -> Linear(1024, 128) -> Tanh) as one fused
forward launch and a fixed-order backward (ops.TowerFn), batch_softmax_loss on its own kernel (ops.BatchSoftmaxFn), the
contrastive term on the InfoNCE kernel and the regulariser on the L2 kernel (util/loss_torch).  The item tower's three
passes of a step -- plain, dropout view 1, dropout view 2 -- are ONE 3B-row problem, so their weight gradients are summed
inside the tower's row reduction and the item table receives all three in one deterministic scatter.  The dropout masks
are drawn in-kernel from the counter RNG (seed, counter, row, column); ``masks`` replays given ones.

Attribute names (user_tower, item_tower, dropout, initial_user_emb, initial_item_emb, query_emb, item_emb,
best_query_emb, best_item_emb) are the reference's, and the parameters are created in its order, so ``torch.manual_seed``
reproduces its initial weights and state_dict keys line up."""
import numpy as np
import torch
import torch.nn as nn

from ... import ops
from ...base.graph_recommender import GraphRecommender
from ...util.loss_torch import InfoNCE, batch_softmax_loss, l2_reg_loss


def _tower_params(tower):
    return tower[0].weight, tower[0].bias, tower[2].weight, tower[2].bias


def _ids(idx):
    """host int64 array of a list / array / tensor of ids"""
    if isinstance(idx, torch.Tensor):
        return idx.detach().cpu().numpy().astype(np.int64)
    return np.asarray(idx, dtype=np.int64).reshape(-1)


class SSL4Rec(GraphRecommender):
    def __init__(self, conf, training_set, test_set):
        super(SSL4Rec, self).__init__(conf, training_set, test_set)
        args = self.config['SSL4Rec']
        self.cl_rate = float(args['alpha'])
        self.tau = float(args['tau'])
        self.drop_rate = float(args['drop'])
        self.model = DNN_Encoder(self.data, self.emb_size, self.drop_rate, self.tau)

    # test() ranks on the device with these (128-wide): the reference's query_emb / item_emb
    @property
    def user_emb(self):
        return getattr(self, 'query_emb', None)

    def batch_losses(self, query_idx, item_idx, masks=None):
        """(rec_loss, cl_loss, batch_loss) of one batch, SSL4Rec.py:31-34 in its order"""
        model = self.model
        query_emb, item_emb, (view1, view2) = model.encode_batch(query_idx, item_idx, masks)
        rec_loss = batch_softmax_loss(query_emb, item_emb, self.tau)
        cl_loss = self.cl_rate * InfoNCE(view1, view2, self.tau)
        batch_loss = rec_loss + l2_reg_loss(self.reg, query_emb, item_emb) + cl_loss
        return rec_loss, cl_loss, batch_loss

    def train(self):
        from ...util.sampler import next_batch_pairwise
        model = self.model.cuda()
        optimizer = torch.optim.Adam(model.parameters(), lr=self.lRate)
        for epoch in range(self.maxEpoch):
            for n, batch in enumerate(next_batch_pairwise(self.data, self.batch_size, as_arrays=True)):
                query_idx, item_idx, _neg = batch
                model.train()
                rec_loss, cl_loss, batch_loss = self.batch_losses(query_idx, item_idx)
                optimizer.zero_grad()
                batch_loss.backward()
                optimizer.step()
                if n % 100 == 0:
                    print('training:', epoch + 1, 'batch', n, 'rec_loss:', rec_loss.item(), 'cl_loss', cl_loss.item())
            model.eval()
            with torch.no_grad():
                self.query_emb, self.item_emb = self.model(None, None)
            self.fast_evaluation(epoch)
        self.query_emb, self.item_emb = self.best_query_emb, self.best_item_emb

    def save(self):
        with torch.no_grad():
            self.best_query_emb, self.best_item_emb = self.model.forward(None, None)

    def predict(self, u):
        u = self.data.get_user_id(u)
        with torch.no_grad():
            score = torch.matmul(self.query_emb[u], self.item_emb.transpose(0, 1))
        return score.cpu().numpy()


class DNN_Encoder(nn.Module):
    def __init__(self, data, emb_size, drop_rate, temperature):
        super(DNN_Encoder, self).__init__()
        self.data = data
        self.emb_size = emb_size
        self.tau = temperature
        self.user_tower = nn.Sequential(
            nn.Linear(self.emb_size, 1024),
            nn.ReLU(True),
            nn.Linear(1024, 128),
            nn.Tanh()
        )
        self.item_tower = nn.Sequential(
            nn.Linear(self.emb_size, 1024),
            nn.ReLU(True),
            nn.Linear(1024, 128),
            nn.Tanh()
        )
        self.dropout = nn.Dropout(drop_rate)
        initializer = nn.init.xavier_uniform_
        self.initial_user_emb = nn.Parameter(initializer(torch.empty(self.data.user_num, self.emb_size)))
        self.initial_item_emb = nn.Parameter(initializer(torch.empty(self.data.item_num, self.emb_size)))
        # the in-kernel dropout masks: view v of a step draws row r at counter rng_counter + v * B + r
        self.rng_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self.rng_counter = 0

    def _tower(self, which, table, ids, **kw):
        dev = table.device
        if ids is None:
            return ops.TowerFn.apply(table, *_tower_params(which), None, None, None, None, 0.0, 0, 0, None)
        idx = torch.from_numpy(ids).to(dev)
        return ops.TowerFn.apply(table, *_tower_params(which), idx, ops.scatter_plan(ids, dev), kw.get('mask_row0'),
                                 kw.get('mask'), kw.get('drop_p', 0.0), self.rng_seed, kw.get('counter', 0),
                                 kw.get('keep_out'))

    def forward(self, q, x):
        """tower outputs of user ids q and item ids x (None: every row of the table), no dropout"""
        q_emb = self._tower(self.user_tower, self.initial_user_emb, None if q is None else _ids(q))
        i_emb = self._tower(self.item_tower, self.initial_item_emb, None if x is None else _ids(x))
        return q_emb, i_emb

    def encode_batch(self, q, x, masks=None, keep_out=None):
        """(query_emb, item_emb, (view1, view2)) of a training batch: the user tower over q and the item tower over
        [x; dropout(x); dropout(x)] as one problem.  masks: optional (2, B, 64) keep flags to replay (1 = keep)."""
        q, x = _ids(q), _ids(x)
        B = int(x.size)
        q_emb = self._tower(self.user_tower, self.initial_user_emb, q)
        mask = None
        if masks is not None:
            mask = torch.as_tensor(masks).to(device=self.initial_item_emb.device, dtype=torch.uint8).reshape(2 * B, -1)
        y = self._tower(self.item_tower, self.initial_item_emb, np.concatenate([x, x, x]), mask_row0=B, mask=mask,
                        drop_p=float(self.dropout.p), counter=self.rng_counter, keep_out=keep_out)
        if mask is None:
            self.rng_counter += 2 * B
        i_emb, i1_emb, i2_emb = y[:B], y[B:2 * B], y[2 * B:]
        return q_emb, i_emb, (i1_emb, i2_emb)

    def item_encoding(self, x):
        """the two dropout views of the item rows x: one 2B-row problem of the item tower"""
        x = _ids(x)
        B = int(x.size)
        y = self._tower(self.item_tower, self.initial_item_emb, np.concatenate([x, x]), mask_row0=0,
                        drop_p=float(self.dropout.p), counter=self.rng_counter)
        self.rng_counter += 2 * B
        return y[:B], y[B:]

    def cal_cl_loss(self, idx):
        item_view1, item_view_2 = self.item_encoding(idx)
        cl_loss = InfoNCE(item_view1, item_view_2, self.tau)
        return cl_loss
