"""float64 restatement of SSL4Rec's step (reference model/graph/SSL4Rec.py:25-46, util/loss_torch.py) -- TEST
INFRASTRUCTURE ONLY, written from the reference's expressions; the product never imports this module.

    tower(x)            tanh(W2 relu(W1 x + b1) + b2)
    batch_softmax       mean_b -log(p_bb + 1e-5),  p = softmax(normalize(U) normalize(V)^T / tau, dim=1)
    InfoNCE             -mean_b log_softmax(normalize(V1) normalize(V2)^T / tau, dim=1)[b, b]
    l2_reg_loss         reg * sum_k ||X_k||_F / rows_k   (unsquared)
    dropout             x * keep / (1 - p)

and the layout of the in-kernel dropout masks (include/selfrec_hip.h, srh_tower_fwd_f32): row r of a view draws at
counter counter0 + r in the counter RNG of tests/counter_rng.py, keep = u01 >= p; view v of a step starts at
counter0 = step_counter + v * B."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import counter_rng

TOWER_KEYS = ("0.weight", "0.bias", "2.weight", "2.bias")


def batch_softmax(u, v, tau):
    u, v = F.normalize(u, dim=1), F.normalize(v, dim=1)
    s = u @ v.T / tau
    p = torch.softmax(s, dim=1).diagonal()
    return (-torch.log(p + 1e-5)).mean()


def infonce(v1, v2, tau):
    v1, v2 = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
    return -torch.diagonal(F.log_softmax(v1 @ v2.T / tau, dim=1)).mean()


def l2_reg(reg, *xs):
    return reg * sum(torch.linalg.vector_norm(x) / x.shape[0] for x in xs)


def tower(x, w1, b1, w2, b2):
    return torch.tanh(torch.relu(x @ w1.T + b1) @ w2.T + b2)


def dropout_keep(seed, counter0, rows, p, d=64):
    """(rows, d) bool: the keep mask the kernel draws for rows counter0, counter0 + 1, ..."""
    return counter_rng.counter_noise(seed, counter0, rows, d) >= np.float32(p)


def step_losses(params, q_idx, i_idx, keep, conf, reg):
    """(rec, cl, total) in float64 for params {name: leaf tensor} (names of DNN_Encoder.named_parameters()); keep:
    (2, B, 64) bool masks of the two views"""
    tau, alpha, drop = float(conf["tau"]), float(conf["alpha"]), float(conf["drop"])
    ut = [params[f"user_tower.{k}"] for k in TOWER_KEYS]
    it = [params[f"item_tower.{k}"] for k in TOWER_KEYS]
    q_idx, i_idx = torch.as_tensor(q_idx, dtype=torch.long), torch.as_tensor(i_idx, dtype=torch.long)
    q = tower(params["initial_user_emb"][q_idx], *ut)
    x = params["initial_item_emb"][i_idx]
    i = tower(x, *it)
    scale = 1.0 / (1.0 - drop)
    k = torch.as_tensor(np.asarray(keep), dtype=x.dtype, device=x.device)
    v1, v2 = tower(x * k[0] * scale, *it), tower(x * k[1] * scale, *it)
    rec = batch_softmax(q, i, tau)
    cl = alpha * infonce(v1, v2, tau)
    return rec, cl, rec + l2_reg(reg, q, i) + cl
