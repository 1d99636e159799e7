"""MHCN (Yu et al., WWW'21; reference model/graph/MHCN.py:13-209, a TF1 graph there), op-level tier: multi-channel
hypergraph convolution for social recommendation.  Config block ``MHCN: {n_layer, ss_rate}`` and the ``social.data`` file.

Three motif-induced hypergraph channels (social H_s, joint H_j, purchase H_p; ``build_hyper_adj_mats``, host scipy, the
reference's arithmetic) and a simple channel over the row-normalised interaction matrix R all start from a self-gated copy
of the user table.  Per layer the three channels are mixed by channel attention (from the UN-normalised channel rows, plus
half the simple channel) to drive the item convolution over R^T; every channel keeps its raw propagated rows for the next
layer and adds their l2_normalize to its sum (MHCN.py:118-138).  The final user rows are the attention mix of the three
sums plus half the simple sum; three more gates of them feed the hierarchical mutual-information loss of each channel.

What runs where:
  * the seven gates x * sigmoid(x W + b): ``ops.GateFn`` (csrc/mhcn.hip: every gate of a call from one read of x, the
    product on the f32 MFMA)                                  (``engine.gate: torch`` / ``SRH_MHCN_GATE``);
  * channel attention: ``ops.ChanMixFn``, one wave per row, with q = attention_mat @ attention^T formed in torch so that
    autograd carries dq to both parameters                    (``engine.mix: torch`` / ``SRH_MHCN_MIX``);
  * hierarchical_self_supervision: ``ops.MimFn``, forward and backward in one call, no float atomics; edge = H @ em is the
    HIP SpMM outside the call                                 (``engine.mim: torch`` / ``SRH_MHCN_MIM``);
  * every sparse product: the HIP SpMM behind ``torch.sparse.mm`` (backward on the explicit transpose); every per-layer
    l2_normalize: ``ops.RowsL2NormFn`` (the SEPT row-normalise kernels);
  * bpr_loss of util/loss_tf.py and the regulariser reg * sum |w|^2 / 2 over every gate / attention weight and the three
    batch embeddings (MHCN.py:184-188): element-wise torch.
The torch routes are the reference's expressions on the same device, the A/B partners of tools/mhcn_probe.py.

Stated deviations from the reference: ``torch.optim.Adam`` adds eps to sqrt(v_hat) where TF1's AdamOptimizer adds it to
sqrt(v) before the bias correction; the initial values and the per-step shuffles come from torch's RNG (xavier_uniform_,
``torch.randperm`` on a seeded device generator), not TF's; the MIM loss is written softplus(-x) =
max(-x, 0) + log1p(exp(-|x|)) where the reference writes -log(sigmoid(x)), which is inf in float32 once x is below about
-88: the two are equal wherever the reference's is finite."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...base.torch_interface import TorchGraphInterface
from ...data.social import Relation
from ...util.route import route
from ._oplevel import OpLevelRecommender
from .SEPT import l2_normalize, tf_bpr_loss

N_CHANNEL = 4                         # MHCN.py:59


def gate_route(conf=None):
    """'hip' or 'torch': SRH_MHCN_GATE, else the conf's engine.gate, else the kernels"""
    return route('SRH_MHCN_GATE', 'engine.gate', conf)


def mix_route(conf=None):
    """'hip' or 'torch': SRH_MHCN_MIX, else the conf's engine.mix, else the kernels"""
    return route('SRH_MHCN_MIX', 'engine.mix', conf)


def mim_route(conf=None):
    """'hip' or 'torch': SRH_MHCN_MIM, else the conf's engine.mim, else the kernels"""
    return route('SRH_MHCN_MIM', 'engine.mim', conf)


def row_normalized(mat):
    """every row over its row sum (MHCN.py:49); an empty row stays empty: its 1 / 0 meets no stored entry"""
    with np.errstate(divide='ignore'):
        return mat.multiply(1.0 / mat.sum(axis=1).reshape(-1, 1))


def hyper_adj_mats(social_mat, interaction_mat):
    """MHCN.py:27-55: [H_s, H_j, H_p] from the directed trust matrix S and the interaction matrix Y.  B = S (.) S^T holds
    the mutual pairs, U = S - B the one-way ones; A1..A7 count the seven triangle motifs of the social graph, A8 / A9 the
    mutual / one-way pairs that share an item, A10 the users who share more than three items and are no friends.  Host scipy
    in float32, the reference's arithmetic term for term."""
    S, Y = social_mat, interaction_mat
    B = S.multiply(S.T)
    U = S - B
    UU, BU, UB, BB = U.dot(U), B.dot(U), U.dot(B), B.dot(B)
    UUt, UtU = U.dot(U.T), U.T.dot(U)
    C1 = UU.multiply(U.T)
    A1 = C1 + C1.T
    C2 = BU.multiply(U.T) + UB.multiply(U.T) + UU.multiply(B)
    A2 = C2 + C2.T
    C3 = BB.multiply(U) + BU.multiply(B) + UB.multiply(B)
    A3 = C3 + C3.T
    A4 = BB.multiply(B)
    C5 = UU.multiply(U) + UUt.multiply(U) + UtU.multiply(U)
    A5 = C5 + C5.T
    A6 = UB.multiply(U) + B.dot(U.T).multiply(U.T) + UtU.multiply(B)
    A7 = U.T.dot(B).multiply(U.T) + BU.multiply(U) + UUt.multiply(B)
    YY = Y.dot(Y.T)
    A8 = YY.multiply(B)
    A9 = YY.multiply(U)
    A9 = A9 + A9.T
    A10 = YY - A8 - A9
    H_s = row_normalized(sum([A1, A2, A3, A4, A5, A6, A7]))
    H_j = row_normalized(sum([A8, A9]))
    H_p = row_normalized(A10.multiply(A10 > 3))
    return [H_s, H_j, H_p]


def gate_torch(x, w, b):
    """MHCN.py:79-83: x * sigmoid(x W + b)"""
    return x * torch.sigmoid(x @ w + b)


def chan_mix_torch(channels, attention, attention_mat):
    """MHCN.py:85-93 as the reference writes it -> (mixed rows, scores (n x 3))"""
    weights = [(attention * (e @ attention_mat)).sum(dim=1) for e in channels]
    score = torch.softmax(torch.stack(weights, dim=1), dim=1)
    mixed = 0
    for i, e in enumerate(channels):
        mixed = mixed + score[:, i:i + 1] * e
    return mixed, score


def mim_torch(em, edge, perms):
    """MHCN.py:159-181 with the shuffles given: perms = (p1, p2, p3 row permutations, c2, c3 column permutations);
    softplus(-x) for -log(sigmoid(x))"""
    p1, p2, p3, c2, c3 = (p.long() for p in perms)
    score = lambda a, b: (a * b).sum(dim=1)  # noqa: E731
    pos = score(em, edge)
    neg1 = score(em[p1], edge)
    neg2 = score(edge[:, c2][p2], em)
    local = (F.softplus(neg1 - pos) + F.softplus(neg2 - neg1)).sum()
    graph = edge.mean(dim=0)
    return local + F.softplus(score(edge[:, c3][p3], graph) - score(edge, graph)).sum()


class MHCN_Encoder(nn.Module):
    """The reference's variables under the reference's names, created in its order, and the four device matrices."""

    def __init__(self, data, emb_size, n_layers, hyper_mats, routes):
        super().__init__()
        self.data, self.n_layers = data, int(n_layers)
        self.gate, self.mix = routes
        xavier = lambda *shape: nn.Parameter(nn.init.xavier_uniform_(torch.empty(*shape)))  # noqa: E731
        self.user_embeddings = xavier(data.user_num, emb_size)
        self.item_embeddings = xavier(data.item_num, emb_size)
        self.weights = nn.ParameterDict()
        for i in range(1, N_CHANNEL + 1):          # (sgating4 / sgating_bias4 are read by nothing but the regulariser)
            self.weights['gating%d' % i] = xavier(emb_size, emb_size)
            self.weights['gating_bias%d' % i] = xavier(1, emb_size)
            self.weights['sgating%d' % i] = xavier(emb_size, emb_size)
            self.weights['sgating_bias%d' % i] = xavier(1, emb_size)
        self.weights['attention'] = xavier(1, emb_size)
        self.weights['attention_mat'] = xavier(emb_size, emb_size)
        convert = TorchGraphInterface.convert_sparse_mat_to_tensor
        self.H = [convert(m).cuda() for m in hyper_mats]
        self.R = convert(data.normalize_graph_mat(data.interaction_mat)).cuda()
        self.attention_score = None

    def gates(self, x, prefix, count):
        w = [self.weights['%s%d' % (prefix, i)] for i in range(1, count + 1)]
        b = [self.weights['%s_bias%d' % (prefix, i)] for i in range(1, count + 1)]
        if self.gate == 'hip':
            return ops.GateFn.apply(x, torch.stack(w), torch.cat(b, dim=0)).unbind(0)
        return tuple(gate_torch(x, wi, bi) for wi, bi in zip(w, b))

    def channel_attention(self, channels, simple):
        """(mix of the three channels + simple / 2, scores)"""
        att, mat = self.weights['attention'], self.weights['attention_mat']
        if self.mix == 'hip':
            q = (mat @ att.T).reshape(-1)          # reduce_sum(att (.) (E M), 1) = E (M att^T)
            return ops.ChanMixFn.apply(channels[0], channels[1], channels[2], q, simple, 0.5)
        mixed, score = chan_mix_torch(channels, att, mat)
        return mixed + simple / 2, score

    def forward(self):
        """MHCN.py:104-148 -> (final user rows, final item rows)"""
        c1, c2, c3, simple = self.gates(self.user_embeddings, 'gating', 4)
        chans = [c1, c2, c3]
        sums = [c1, c2, c3]
        simple_sum, item, item_sum = simple, self.item_embeddings, self.item_embeddings
        norm = ops.RowsL2NormFn.apply
        r_t = self.R.transposed()
        for _ in range(self.n_layers):
            mixed, _score = self.channel_attention(chans, simple)
            chans = [torch.sparse.mm(h, c) for h, c in zip(self.H, chans)]
            sums = [s + norm(c) for s, c in zip(sums, chans)]
            new_item = torch.sparse.mm(r_t, mixed)
            item_sum = item_sum + norm(new_item)
            simple = torch.sparse.mm(self.R, item)
            simple_sum = simple_sum + norm(simple)
            item = new_item
        user, self.attention_score = self.channel_attention(sums, simple_sum)
        return user, item_sum


class MHCN(OpLevelRecommender):
    def __init__(self, conf, training_set, test_set, **kwargs):
        super().__init__(conf, training_set, test_set, **kwargs)
        args = self.config['MHCN']
        self.n_layers = int(args['n_layer'])
        self.ss_rate = float(args['ss_rate'])
        self.social_data = Relation(conf, kwargs['social.data'], self.data.user)
        self.gate, self.mix, self.mim = gate_route(conf), mix_route(conf), mim_route(conf)
        self.model = MHCN_Encoder(self.data, self.emb_size, self.n_layers, self.build_hyper_adj_mats(),
                                  (self.gate, self.mix))
        self.shuffle_seed = 2024
        self.generator = None
        self.draw_perms = None         # hook: draw_perms(channel, n, d, device) -> (p1, p2, p3, c2, c3); None: the generator
        self.optimizer = None

    def print_model_info(self):
        super().print_model_info()
        print('Social data size: (user number: %d, relation number: %d).' % (self.social_data.size()))
        print('=' * 80)

    @property
    def attention_score(self):
        """the channel scores (users x 3) of the last forward pass's final mix (MHCN.py:147)"""
        return self.model.attention_score

    def build_hyper_adj_mats(self):
        return hyper_adj_mats(self.social_data.get_social_mat(), self.data.interaction_mat)

    def perms(self, channel, n, d, device):
        """the five shuffles of one hierarchical_self_supervision call (MHCN.py:160-165), fresh on every call"""
        if self.draw_perms is not None:
            return tuple(torch.as_tensor(p).to(device=device, dtype=torch.int32) for p in self.draw_perms(channel, n, d, device))
        if self.generator is None or self.generator.device.type != torch.device(device).type:
            self.generator = torch.Generator(device=device)
            self.generator.manual_seed(self.shuffle_seed)
        draw = lambda m: torch.randperm(m, generator=self.generator, device=device).to(torch.int32)  # noqa: E731
        p1, c2, p2, c3, p3 = draw(n), draw(d), draw(n), draw(d), draw(n)       # the order the reference draws them in
        return p1, p2, p3, c2, c3

    def mim_loss(self, em, adj, channel):
        edge = torch.sparse.mm(adj, em)
        perms = self.perms(channel, int(em.shape[0]), int(em.shape[1]), em.device)
        if self.mim == 'hip':
            return ops.MimFn.apply(em, edge, *perms)
        return mim_torch(em, edge, perms)

    def batch_losses(self, user_idx, pos_idx, neg_idx):
        """(rec_loss, reg_loss, ss_loss (ss_rate applied), their sum) of one batch, MHCN.py:150-153 and 184-189"""
        model = self.model
        user, item = model()
        ss = 0
        for ch, em in enumerate(model.gates(user, 'sgating', 3)):
            ss = ss + self.mim_loss(em, model.H[ch], ch)
        ss_loss = self.ss_rate * ss
        bu, bp, bn = user[user_idx], item[pos_idx], item[neg_idx]
        rec_loss = tf_bpr_loss(bu, bp, bn)
        reg = sum((w ** 2).sum() / 2 for w in model.weights.values())
        reg = reg + ((bu ** 2).sum() + (bn ** 2).sum() + (bp ** 2).sum()) / 2
        reg_loss = self.reg * reg
        return rec_loss, reg_loss, ss_loss, rec_loss + reg_loss + ss_loss

    def train(self):
        from ...util.sampler import next_batch_pairwise
        model = self.model.cuda()
        self.optimizer = torch.optim.Adam(list(model.parameters()), lr=self.lRate)
        self.rec_loss_history = []     # per epoch: the recommendation loss per training sample (one read-back per epoch)
        for epoch in range(self.maxEpoch):
            model.train()
            rec_sum = torch.zeros((), device='cuda')
            for n, batch in enumerate(next_batch_pairwise(self.data, self.batch_size, as_arrays=True)):
                user_idx, pos_idx, neg_idx = (torch.from_numpy(a).cuda() for a in batch)
                rec_loss, _reg, ss_loss, loss = self.batch_losses(user_idx, pos_idx, neg_idx)
                self.optimizer.zero_grad()
                loss.backward()
                self.optimizer.step()
                rec_sum += rec_loss.detach()
                if n % self.verbose_every == 0 and n > 0:
                    print('training:', epoch + 1, 'batch', n, 'rec loss:', rec_loss.item(), 'ssl loss', ss_loss.item())
            self.rec_loss_history.append(rec_sum.item() / max(len(self.data.training_data), 1))
            model.eval()
            with torch.no_grad():
                self.snapshot()
            self.fast_evaluation(epoch)
        self.restore_best()

    def snapshot(self):
        self.user_emb, self.item_emb = self.model()
