"""The kernel cases of CL4SRec's tests -- TEST INFRASTRUCTURE ONLY.  tests/test_gpu_cl4srec.py runs the kernels on them;
tests/test_cl4srec_cpu.py runs float32 torch on the same cases against the same float64 references and bounds, which shows
that the bounds are float32's to meet.  Every case is computed once (lru_cache) and never modified."""
import functools

import numpy as np
import torch

from tests import cl4srec_ref

CHUNK = 32                                   # SRH_LIVE_SUM_CHUNK
EMBED_SHAPES = [(1, 1, 64), (3, 7, 32), (5, 50, 64), (4, 64, 128), (768, 50, 64)]
DROP_P = 0.2
N_ITEMS = 40                                 # item ids 1 .. 40, the mask token 41: tables of 42 rows
REPEATED = 7                                 # the id every live sequence starts with
SEGMENT_LENGTHS = [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 20 * CHUNK + 3]
NCE_SIZES = [1, 2, 24, 256]
OUT_BOUND, GRAD_BOUND = 1e-5, 1e-4           # of the tensor's largest magnitude


def rel_err(got, want):
    """largest error as a fraction of the tensor's largest magnitude"""
    want = torch.as_tensor(want).double().cpu()
    return float((torch.as_tensor(got).double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def shape_id(s):
    return "B%d_L%d_d%d" % s


@functools.lru_cache(maxsize=None)
def embed_case(shape):
    """ids of a right-padded batch with every special row, both tables, a keep mask, an upstream gradient whose dead rows
    are NaN, and the float64 outputs and table gradients with and without the mask"""
    B, L, d = shape
    rs = np.random.RandomState(100 * B + L + d)
    lens = rs.randint(1, L + 1, size=B)
    if B > 1:
        lens[1] = 0                                               # one sequence is all padding
    seq, pos = np.zeros((B, L), dtype=np.int32), np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        n = int(lens[b])
        seq[b, :n] = rs.randint(1, N_ITEMS + 1, size=n)
        pos[b, :n] = np.arange(1, n + 1)
        if n:
            seq[b, 0] = REPEATED                                  # one id in every row
        if n > 2:
            seq[b, n // 2] = N_ITEMS + 1                          # the mask token
        if n < L:
            pos[b, n:] = rs.randint(0, L + 1, size=L - n)         # seq = 0 with pos != 0
    g = torch.Generator().manual_seed(B + 10 * L + d)
    item = torch.randn(N_ITEMS + 2, d, generator=g)
    pos_table = torch.randn(L + 1, d, generator=g)
    keep = torch.rand(B * L, d, generator=g) >= DROP_P
    go = torch.randn(B * L, d, generator=g)
    live = seq.reshape(-1) != 0
    go_nan = go.clone()
    go_nan[torch.from_numpy(~live)] = float('nan')
    c = dict(seq=seq, pos=pos, item=item, pos_table=pos_table, keep=keep, go=go, go_nan=go_nan, live=live)
    i64, p64 = item.double(), pos_table.double()
    c["out"] = cl4srec_ref.embed_front(i64, p64, seq, pos)
    c["out_keep"] = cl4srec_ref.embed_front(i64, p64, seq, pos, keep.numpy(), DROP_P)
    x = go.numpy()
    for tag, mult in (("", None), ("_keep", keep.numpy() / (1.0 - DROP_P))):
        c["gi" + tag] = cl4srec_ref.live_sum(x, seq, live, N_ITEMS + 2, d ** 0.5, mult)
        c["gp" + tag] = cl4srec_ref.live_sum(x, pos, live, L + 1, 1.0, mult)
    return c


@functools.lru_cache(maxsize=None)
def segment_case(d=64):
    """one segment of every length in SEGMENT_LENGTHS, their rows interleaved at random among dead rows (NaN): ids, live,
    x, and the float64 sums"""
    rs = np.random.RandomState(5)
    ids = np.concatenate([np.full(n, 3 + 2 * k) for k, n in enumerate(SEGMENT_LENGTHS)] + [np.zeros(300, dtype=np.int64)])
    live = np.r_[np.ones(sum(SEGMENT_LENGTHS), dtype=bool), np.zeros(300, dtype=bool)]
    order = rs.permutation(ids.size)
    ids, live = ids[order], live[order]
    ids[~live] = rs.randint(0, 20, size=int((~live).sum()))        # a dead row's id names nothing
    x = torch.randn(ids.size, d, generator=torch.Generator().manual_seed(6))
    n_table = 3 + 2 * len(SEGMENT_LENGTHS)
    want = cl4srec_ref.live_sum(x.numpy(), ids, live, n_table)
    x_nan = x.clone()
    x_nan[torch.from_numpy(~live)] = float('nan')
    return dict(ids=ids, live=live, x=x, x_nan=x_nan, n_table=n_table, want=want)


@functools.lru_cache(maxsize=None)
def nce_case(n, d=64):
    g = torch.Generator().manual_seed(n)
    v1, v2 = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
    a, b = v1.double().requires_grad_(True), v2.double().requires_grad_(True)
    loss = cl4srec_ref.info_nce(a, b, 1.0)
    loss.backward()
    return dict(v1=v1, v2=v2, loss=float(loss.detach()), g1=a.grad, g2=b.grad)


def torch_embed_front(item, pos_table, seq, pos, keep=None, drop_p=0.0):
    """the torch route's expression (SASRec_Model.forward's front) on tensors of any device and dtype"""
    seq_t = torch.as_tensor(np.asarray(seq).reshape(-1), device=item.device).long()
    pos_t = torch.as_tensor(np.asarray(pos).reshape(-1), device=item.device).long()
    x = item[seq_t] * item.shape[1] ** 0.5 + pos_table[pos_t]
    if keep is not None:
        x = x * (keep.to(x.dtype) / (1.0 - drop_p))
    return x * (seq_t != 0).unsqueeze(-1)
