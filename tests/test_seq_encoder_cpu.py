"""What SASRec, BERT4Rec and CL4SRec share (model/sequential/encoder.py, util/route.py) without a GPU: the one upload and
its views, the three staged batch types cut from it, the one route helper behind the six public switches, and the three
thin encoder classes' parameter names, order, table heights and random draws."""
import json
import os
import types

import numpy as np
import pytest
import torch

from tests.test_shapes_cpu import GOLDEN


def storage_of(t):
    return t.untyped_storage().data_ptr()


def test_upload_returns_views_of_one_tensor_and_takes_empty_arrays():
    from selfrec_amd import ops
    from selfrec_amd.model.sequential.encoder import upload, upload_with_plans
    ids = np.array([[3, 0, 7], [7, 7, 0]], dtype=np.int64)
    plan = ops.live_plan_host(ids)                           # no id fills a second chunk: two empty arrays
    assert [a.size for a in plan[3:]] == [0, 0] and plan[0].size == 4
    arrays = [ids, np.zeros(0, dtype=np.int32), np.arange(5, dtype=np.int32), *plan]
    views = upload(arrays, torch.device("cpu"))
    assert len(views) == len(arrays)
    for v, a in zip(views, arrays):
        assert v.dtype == torch.int32 and v.dim() == 1 and np.array_equal(v.numpy(), np.asarray(a).reshape(-1))
    assert len({storage_of(v) for v in views}) == 1          # one tensor: one host-to-device copy
    assert [v.storage_offset() for v in views] == np.r_[0, np.cumsum([a.size for a in arrays])[:-1]].tolist()
    head, plans = upload_with_plans([ids, ids], [ops.scatter_plan_host(ids), plan], torch.device("cpu"))
    assert len(head) == 2 and [len(p) for p in plans] == [3, 5]
    for got, want in zip(plans, (ops.scatter_plan_host(ids), plan)):
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    assert len({storage_of(v) for v in head + [a for p in plans for a in p]}) == 1


def test_staged_batches_are_one_upload_with_the_plans_of_their_ids():
    from selfrec_amd import ops
    from selfrec_amd.model.sequential.BERT4Rec import StagedMaskedBatch
    from selfrec_amd.model.sequential.CL4SRec import StagedViews
    from selfrec_amd.model.sequential.encoder import Group
    from selfrec_amd.model.sequential.SASRec import StagedBatch
    cpu = torch.device("cpu")
    seq = np.array([[4, 9, 4, 0], [2, 0, 0, 0], [9, 9, 9, 9]])
    pos = np.where(seq != 0, np.arange(1, 5)[None, :], 0)
    y, neg = np.roll(seq, 1, axis=1) * (seq != 0), (seq + 1) * (seq != 0)

    def same(plan, host):
        return len(plan) == len(host) and all(np.array_equal(a.numpy(), b) for a, b in zip(plan, host))

    b = StagedBatch(seq, pos, y, neg, cpu)
    assert b.shape == (3, 4) and b.route_embed == 'torch' and b.n_valid == 8 and b.valid.dtype == torch.uint8
    for got, want in ((b.seq, seq), (b.pos, pos), (b.y, y), (b.neg, neg), (b.valid, pos != 0), (b.live, seq != 0)):
        assert np.array_equal(got.numpy().reshape(-1), want.reshape(-1))
    assert len(b.plans) == 3 and same(b.plans[0], ops.scatter_plan_host(seq)) and same(b.plans[1], ops.scatter_plan_host(pos))
    assert same(b.plans[2], ops.scatter_plan_host(np.concatenate([y.reshape(-1), neg.reshape(-1)])))
    assert len({storage_of(t) for t in [b.seq, b.pos, b.y, b.neg] + [a for p in b.plans for a in p]}) == 1
    g, = b.groups
    assert isinstance(g, Group) and g.seq is b.seq and g.pos is b.pos and g.live is b.live and g.shape == (3, 4)
    bare = StagedBatch(seq, pos, None, None, cpu)
    assert bare.y is None and bare.neg is None and len(bare.plans) == 2 and bare.live.shape == (3, 4, 1)

    masked = np.array([[0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 1]])
    m = StagedMaskedBatch(seq, pos, masked, [9, 2, 9, 9], cpu)
    assert m.n_masked == 4 and m.masked_idx.tolist() == [1, 4, 10, 11] and m.labels.tolist() == [9, 2, 9, 9]
    assert len(m.plans) == 2 and same(m.plans[0], b.plans[0]) and m.groups[0].live.shape == (3, 4, 1)
    assert len({storage_of(t) for t in [m.seq, m.pos, m.masked_idx, m.labels] + [a for p in m.plans for a in p]}) == 1
    bare = StagedMaskedBatch(seq, pos, None, None, cpu)
    assert bare.masked_idx is None and bare.labels is None and bare.n_masked == 0
    with pytest.raises(ValueError):
        StagedMaskedBatch(seq, pos, masked, [9, 2], cpu)

    views = [(seq, pos, None), (seq[:, ::-1].copy(), pos, [3, 1, 4]), (seq, pos, [3, 1, 4])]
    for route_views, route_embed in (("one", "hip"), ("three", "hip"), ("one", "torch"), ("three", "torch")):
        s = StagedViews(views, y, neg, cpu, route_views, route_embed)
        plan_of = ops.live_plan_host if route_embed == "hip" else (lambda ids, live: ops.scatter_plan_host(ids))
        assert len(s.groups) == (1 if route_views == "one" else 3) and s.route_embed == route_embed
        stacked = [np.concatenate([v[k].reshape(-1) for v in views]) for k in (0, 1)]
        rows = 0
        for g in s.groups:
            n = g.shape[0] * g.shape[1]
            ids, places = (a[rows:rows + n] for a in stacked)
            assert np.array_equal(g.seq.numpy(), ids) and np.array_equal(g.pos.numpy(), places)
            assert same(g.plans[0], plan_of(ids, ids != 0)) and same(g.plans[1], plan_of(places, ids != 0))
            assert np.array_equal(g.live.numpy().reshape(-1), ids != 0) and g.live.shape == (*g.shape, 1)
            rows += n
        assert rows == 36 and s.n_valid == 8 and np.array_equal(s.valid.numpy(), pos.reshape(-1) != 0)
        valid2 = np.concatenate([pos.reshape(-1) != 0] * 2)
        assert same(s.bce_plan, plan_of(np.concatenate([y.reshape(-1), neg.reshape(-1)]), valid2))
        base = 3 if route_views == "one" else 0
        assert s.last[0].tolist() == [(base + r) * 4 + n - 1 for r, n in enumerate([3, 1, 4])]
        tensors = [s.y, s.neg, *s.last, *s.bce_plan] + [t for g in s.groups for t in (g.seq, g.pos, *g.plans[0], *g.plans[1])]
        assert len({storage_of(t) for t in tensors}) == 1


ROUTES = [("sequential.SASRec", "attention_route", "SRH_SASREC_ATTN", "engine.attention", ("hip", "torch")),
          ("sequential.BERT4Rec", "ce_route", "SRH_BERT4REC_CE", "engine.ce", ("hip", "torch")),
          ("sequential.CL4SRec", "views_route", "SRH_CL4SREC_VIEWS", "engine.views", ("one", "three")),
          ("sequential.CL4SRec", "embed_route", "SRH_CL4SREC_EMBED", "engine.embed", ("hip", "torch")),
          ("graph.SEPT", "nd_route", "SRH_SEPT_ND", "engine.nd", ("hip", "torch")),
          ("graph.SEPT", "norm_route", "SRH_SEPT_NORM", "engine.norm", ("hip", "torch"))]


@pytest.mark.parametrize("module,name,env,key,choices", ROUTES, ids=[r[1] for r in ROUTES])
def test_the_six_route_switches_are_the_one_helper(monkeypatch, module, name, env, key, choices):
    import importlib
    from selfrec_amd.util.conf import ModelConf
    from selfrec_amd.util.route import route
    fn = getattr(importlib.import_module(f"selfrec_amd.model.{module}"), name)
    monkeypatch.delenv(env, raising=False)
    assert fn() == fn(None) == fn(ModelConf({})) == choices[0]
    assert fn(ModelConf({key: choices[1]})) == choices[1]
    assert fn(ModelConf({key: f"  {choices[1].upper()} "})) == choices[1]          # lower-cased and stripped
    with pytest.raises(ValueError, match=f"{key} / {env}"):
        fn(ModelConf({key: "eager"}))
    monkeypatch.setenv(env, f" {choices[1].capitalize()}")
    assert fn(ModelConf({key: choices[0]})) == choices[1] == fn(None)             # the environment beats the conf
    assert route(env, key, ModelConf({key: choices[0]}), choices) == choices[1]
    monkeypatch.setenv(env, "")
    with pytest.raises(ValueError):
        fn(ModelConf({key: choices[0]}))                                         # (an empty variable is set, and is no route)


def meta_of(name):
    return json.load(open(os.path.join(GOLDEN, f"{name}_meta.json")))


def test_the_three_encoders_are_one_class_with_the_goldens_parameters():
    from selfrec_amd.model.sequential.BERT4Rec import BERT_Encoder
    from selfrec_amd.model.sequential.CL4SRec import CL4SRec_Model
    from selfrec_amd.model.sequential.encoder import SeqEncoder
    from selfrec_amd.model.sequential.SASRec import SASRec_Model
    nets, after = {}, {}
    for cls, golden in ((SASRec_Model, "sasrec"), (BERT_Encoder, "bert4rec"), (CL4SRec_Model, "cl4srec")):
        meta = meta_of(golden)
        c = meta["conf"]
        torch.manual_seed(7)
        net = cls(types.SimpleNamespace(item_num=meta["item_num"]), c["emb"], c["max_len"], c["n_blocks"], 2, 0.2)
        after[cls] = torch.get_rng_state()
        assert isinstance(net, SeqEncoder) and cls.forward is SeqEncoder.forward and cls._attention is SeqEncoder._attention
        assert [n for n, _ in net.named_parameters()] == meta["param_names"] == list(net.state_dict())
        extra = 1 if cls is SASRec_Model else 2
        assert net.item_emb.shape == (meta["item_num"] + extra, c["emb"])
        assert net.pos_emb.shape == (c["max_len"] + (2 if cls is BERT_Encoder else 1), c["emb"])
        assert 0 <= net.rng_seed < 2 ** 62 and net.rng_counter == 0
        nets[cls] = net
    sas, bert, cl = nets[SASRec_Model], nets[BERT_Encoder], nets[CL4SRec_Model]
    assert issubclass(CL4SRec_Model, SASRec_Model) and not issubclass(BERT_Encoder, SASRec_Model)
    assert sas.causal and cl.causal and not bert.causal
    assert [type(f.pwff[1]).__name__ for f in bert.forward_layers] == ["GELU", "GELU"]
    assert [type(f.pwff[1]).__name__ for f in sas.forward_layers] == ["ReLU", "ReLU"]
    # CL4SRec draws SASRec's network first, then its own table, then the one rng_seed: everything but the table is
    # SASRec's bit for bit, and the seed comes from further down the stream
    for (name, p), (_, q) in zip(sas.named_parameters(), cl.named_parameters()):
        assert name == "item_emb" or torch.equal(p, q), name
    assert sas.rng_seed != cl.rng_seed
    # one draw per model and nothing behind it: the generator stands where a replay of the draws leaves it
    torch.manual_seed(7)
    SASRec_Model(types.SimpleNamespace(item_num=80), 64, 12, 2, 2, 0.2)
    assert torch.equal(torch.get_rng_state(), after[SASRec_Model])
    torch.nn.init.xavier_uniform_(torch.empty(1, 1))
    assert not torch.equal(torch.get_rng_state(), after[SASRec_Model])


def test_attention_functions_keep_their_names_and_the_bce_pair_shares_a_forward():
    from selfrec_amd import ops
    for name in ("SeqAttnFn", "SeqAttnFullFn", "SeqBceFn", "SeqBceLiveFn", "seq_attn_fwd", "seq_attn_bwd",
                 "seq_attn_full_fwd", "seq_attn_full_bwd"):
        assert name in ops.__all__ and getattr(ops, name), name
    assert callable(ops.SeqAttnFn.apply) and callable(ops.SeqAttnFullFn.apply)
    assert ops.SeqBceLiveFn.forward is ops.SeqBceFn.forward and issubclass(ops.SeqBceLiveFn, torch.autograd.Function)
    assert ops.SeqBceLiveFn.table_grad is not ops.SeqBceFn.table_grad
