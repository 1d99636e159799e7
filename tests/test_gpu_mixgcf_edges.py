"""The hop-mixing kernels at the ends of what they serve: no pairs, the refused shapes, wrong operands, and a backward
pass whose every row sums many contributions run twice."""
import numpy as np
import pytest
import torch

from tests import mixgcf_cases as mc

pytestmark = pytest.mark.gpu


def tensors(B, H, C, d, n_items, seed=5):
    g = torch.Generator().manual_seed(seed)
    hops = [(0.1 * torch.randn(n_items, d, generator=g)).cuda() for _ in range(H)]
    u = (0.1 * torch.randn(B, d, generator=g)).cuda()
    pos = torch.randint(0, max(n_items, 1), (B,), generator=g).cuda()
    neg = torch.randint(0, max(n_items, 1), (B * C,), generator=g).cuda()
    return u, hops, pos, neg


def test_no_pairs_gives_empty_outputs_and_zero_tables():
    from selfrec_amd import ops
    H, C, d, n_items = 4, 64, 64, 50
    u, hops, pos, neg = tensors(0, H, C, d, n_items)
    pos_out, neg_out, pick = ops.mixup_fwd(u, hops, pos, neg, C)
    assert tuple(pos_out.shape) == (0, d) and tuple(neg_out.shape) == (0, d) and tuple(pick.shape) == (H, 0)
    grads = ops.mixup_bwd(hops, pos, neg, C, pick, torch.empty(0, d).cuda(), torch.empty(0, d).cuda())
    assert len(grads) == H and all(tuple(g.shape) == (n_items, d) and (g == 0).all() for g in grads)


@pytest.mark.parametrize("shape", [(6, 4, 3), (260, 4, 3), (64, 9, 3), (64, 4, 0), (2, 1, 1)],
                         ids=lambda s: "d%d_H%d_C%d" % s)
def test_unsupported_shapes_are_refused_by_the_library(shape):
    from selfrec_amd import ops
    d, H, C = shape
    assert not ops.mixup_supported(d, H, C)
    B, n_items = 3, 20
    u, hops, pos, neg = tensors(B, H, C, d, n_items)
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.mixup_fwd(u, hops, pos, neg, C)
    pick = torch.zeros((H, B), dtype=torch.int32).cuda()
    with pytest.raises(ops.SelfrecHipError, match="unsupported"):
        ops.mixup_bwd(hops, pos, neg, C, pick, u, u)


@pytest.mark.parametrize("shape", [(4, 1, 1), (8, 2, 2), (60, 3, 5), (100, 8, 130), (256, 8, 1), (252, 5, 7)],
                         ids=lambda s: "d%d_H%d_C%d" % s)
def test_mixup_supported_agrees_with_the_library(shape):
    from selfrec_amd import ops
    d, H, C = shape
    assert ops.mixup_supported(d, H, C)
    u, hops, pos, neg = tensors(3, H, C, d, 20)
    pos_out, neg_out, pick = ops.mixup_fwd(u, hops, pos, neg, C)
    assert torch.isfinite(neg_out).all() and int(pick.min()) >= 0 and int(pick.max()) < C
    assert all(tuple(g.shape) == (20, d) for g in ops.mixup_bwd(hops, pos, neg, C, pick, u, u))


def test_wrong_operands_are_refused_by_the_wrapper():
    from selfrec_amd import ops
    B, H, C, d, n_items = 3, 2, 4, 64, 20
    u, hops, pos, neg = tensors(B, H, C, d, n_items)
    pick = torch.zeros((H, B), dtype=torch.int32).cuda()
    with pytest.raises(ops.SelfrecHipError, match="B x d"):
        ops.mixup_fwd(u[:, :32], hops, pos, neg, C)
    with pytest.raises(ops.SelfrecHipError, match="n_negs"):
        ops.mixup_fwd(u, hops, pos, neg[:-1], C)
    with pytest.raises(ops.SelfrecHipError, match="share one"):
        ops.mixup_fwd(u, [hops[0], hops[1][:-1]], pos, neg, C)
    with pytest.raises(ops.SelfrecHipError, match="alpha"):
        ops.mixup_fwd(u, hops, pos, neg, C, alpha=torch.rand(H, B, C, d // 2).cuda())
    with pytest.raises(ops.SelfrecHipError, match="alpha"):
        ops.mixup_fwd(u, hops, pos, neg, C, alpha=[torch.rand(B, C, d).cuda()])
    with pytest.raises(ops.SelfrecHipError, match="pick"):
        ops.mixup_bwd(hops, pos, neg, C, pick[:1], u, u)
    with pytest.raises(ops.SelfrecHipError, match="g_pos"):
        ops.mixup_bwd(hops, pos, neg, C, pick, u[:2], u)
    with pytest.raises(ops.SelfrecHipError, match="HIP device"):
        ops.mixup_fwd(u, hops, pos.cpu(), neg, C)
    with pytest.raises(ops.SelfrecHipError):
        ops.mixup_fwd(u, [h.cpu() for h in hops], pos, neg, C)


@pytest.mark.parametrize("case", [c for c in mc.CASES if c[0] == "collide"], ids=mc.case_id)
def test_colliding_backward_repeats_bit_for_bit(case):
    """I = 3: every row of every gradient table is a sum over many pairs, in one fixed order"""
    from selfrec_amd import ops
    fam, B, H, C, d, n_items = case
    c = mc.inputs(case)
    hops = [torch.from_numpy(t).cuda() for t in c["tables"]]
    u, pos, neg = torch.from_numpy(c["u"]).cuda(), torch.from_numpy(c["pos"]).cuda(), torch.from_numpy(c["neg"]).cuda()
    g_pos, g_neg = torch.from_numpy(c["g_pos"]).cuda(), torch.from_numpy(c["g_neg"]).cuda()
    rng = dict(rng_seed=c["rng_seed"], rng_counter=c["rng_counter"])
    _, _, pick = ops.mixup_fwd(u, hops, pos, neg, C, **rng)
    first = [g.clone() for g in ops.mixup_bwd(hops, pos, neg, C, pick, g_pos, g_neg, **rng)]
    again = ops.mixup_bwd(hops, pos, neg, C, pick, g_pos, g_neg, **rng)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # the order of the sum is ascending pair, positive before negative: float32 numpy in that order gives the same bits
    al = c["alpha"]
    pk = pick.cpu().numpy()
    negs = c["neg"].reshape(B, C)
    want = np.zeros((H, n_items, d), dtype=np.float32)
    hf = np.float32(H)
    for k in range(H):
        started = set()
        for b in range(B):
            a = al[k, b, pk[k, b]]
            # fma(alpha, g_neg, g_pos) / H and ((1 - alpha) g_neg) / H, as the header states them
            sp = ((a.astype(np.float64) * c["g_neg"][b].astype(np.float64) + c["g_pos"][b]).astype(np.float32)) / hf
            sn = ((np.float32(1.0) - a) * c["g_neg"][b]) / hf
            for row, share in ((c["pos"][b], sp), (negs[b, pk[k, b]], sn)):
                want[k, row] = share if row not in started else want[k, row] + share
                started.add(row)
    assert all(np.array_equal(first[k].cpu().numpy(), want[k]) for k in range(H))
