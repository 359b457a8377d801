"""GPU suite for the ablation encoders on the scoring pipeline: the user context on group-shared node features against the per-row
entry, ``util.compute_scores`` for all five classes against the fp32 CPU oracle (oracle/digat_oracle.py: ``ablation_encode``), the
grouped route against the per-row route, a ``Trainer`` dev epoch, and derived user graphs."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle import digat_oracle as O

pytestmark = pytest.mark.gpu

CHOICE = {"wo_SA": "wo_SA", "Seq_SA": "Seq_SA", "wo_interaction": "wo_interaction", "News_graph_wo_inter": "news_graph_wo_inter",
          "User_graph_wo_inter": "user_graph_wo_inter"}          # class name -> --graph_encoder choice (config.py:19)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# 1. digat_user_ctx_fwd_grouped == digat_user_ctx_fwd on the expanded tensors, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _ctx_case(H, C, d, B, G=6, seed=0):
    """Groups: 0 has ONE row, 2 has an empty history (every slot is padding, no category unmasked), 4 has NO row."""
    rng = np.random.default_rng(seed)
    U, C1 = H + C, C + 1
    Xu = rng.standard_normal((G, U, d)).astype(np.float32)
    idx = rng.integers(0, C, size=(G, H)).astype(np.int64)
    for g in range(G):
        idx[g, rng.integers(1, H + 1):] = C                       # right-padded histories of different lengths
    idx[2, :] = C
    mask = np.zeros((G, C1), dtype=bool)
    for g in range(G):
        mask[g, np.unique(idx[g][idx[g] < C])] = True
    users = [1, 2, 3, 5]
    counts = rng.multinomial(B - 1 - len(users), np.ones(len(users)) / len(users)) + 1
    ascending = np.concatenate([[0]] + [np.full(n, g) for g, n in sorted(zip(users, counts))]).astype(np.int32)
    assert ascending.shape == (B,) and 4 not in ascending and (ascending == 0).sum() == 1
    c_n = rng.standard_normal((B, d)).astype(np.float32)
    acc = rng.standard_normal((B, d)).astype(np.float32)
    w = [(rng.standard_normal(s) / np.sqrt(d)).astype(np.float32) for s in ((d, d), (d, d), (d,), (d, d), (d,), (d, d), (d, d), (d,))]
    return Xu, mask, idx, ascending, rng.permutation(ascending), c_n, acc, w


@pytest.mark.parametrize("H,C,d,B", [(10, 5, 64, 37), (50, 17, 400, 96)])
def test_grouped_user_context_is_bit_identical_to_the_expanded_one(H, C, d, B):
    from digat_amd import _lib
    L = _lib.lib()
    dev = _dev()
    Xu, mask, idx, asc, perm, c_n, acc, w = _ctx_case(H, C, d, B, seed=H + d)
    G, U, C1 = Xu.shape[0], H + C, C + 1

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Xu_g, mask_g, idx_g, c_n_t, acc_t = t(Xu), t(mask).view(torch.uint8), t(idx), t(c_n), t(acc)
    wt = [t(x) for x in w]
    wp = [x.data_ptr() for x in wt]
    S = _lib.stream_ptr()
    for name, rg_np in (("ascending", asc), ("permuted", perm)):
        rg = t(rg_np)
        rgl = rg.long()
        Xu_x, mask_x, idx_x = Xu_g.index_select(0, rgl), mask_g.index_select(0, rgl), idx_g.index_select(0, rgl)
        for with_addend in (False, True):
            want = acc_t.clone() if with_addend else torch.full((B, d), float("nan"), device=dev)
            got = want.clone()
            nb = L.digat_user_ctx_workspace_bytes(B, U, H, C1, d)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            _lib.check(L.digat_user_ctx_fwd(Xu_x.data_ptr(), mask_x.data_ptr(), idx_x.data_ptr(), c_n_t.data_ptr(), *wp,
                                            want.data_ptr() if with_addend else None, want.data_ptr(), B, U, H, C1, d,
                                            ws.data_ptr(), nb, S), "digat_user_ctx_fwd")
            ng = L.digat_user_ctx_grouped_workspace_bytes(B, G, U, H, C1, d)
            wsg = torch.empty(ng, dtype=torch.uint8, device=dev)
            _lib.check(L.digat_user_ctx_fwd_grouped(Xu_g.data_ptr(), mask_g.data_ptr(), idx_g.data_ptr(), rg.data_ptr(), c_n_t.data_ptr(),
                                                    *wp, got.data_ptr() if with_addend else None, got.data_ptr(), B, G, U, H, C1, d,
                                                    wsg.data_ptr(), ng, S), "digat_user_ctx_fwd_grouped")
            torch.cuda.synchronize()
            assert torch.isfinite(want).all(), (name, with_addend)
            assert torch.equal(got, want), (name, with_addend, float((got - want).abs().max()))
            if with_addend:
                assert not torch.equal(got, acc_t)


@pytest.mark.parametrize("H,C,d", [(10, 5, 64), (50, 17, 400)])
def test_user_nodes_build_equals_cat_and_expand(H, C, d):
    """digat_user_nodes_build: Xu^(0) per group, and the expanded tensor written directly through a permuted row map."""
    from digat_amd import graphEncoders
    dev = _dev()
    cfg = types.SimpleNamespace(news_graph_size=4, max_history_num=H, category_num=C, graph_depth=1, dropout_rate=0.2)
    enc = graphEncoders.Seq_SA(cfg, d).to(dev).eval()
    g = torch.Generator().manual_seed(d)
    with torch.no_grad():
        enc.topic_node_embedding.copy_(torch.randn(C, d, generator=g))
    G, B = 7, 301                                            # more graphs than one workgroup's stride would need, an odd row count
    ue = torch.randn(G, H, d, generator=g).to(dev)
    rg = torch.randint(0, G, (B,), generator=g).to(torch.int32).to(dev)
    want = enc._user_nodes(ue)                              # the reference-pinned cat + expand
    assert torch.equal(enc._user_nodes_dev(ue), want)
    assert torch.equal(enc._user_nodes_dev(ue, rg), want.index_select(0, rg.long()))


# ---------------------------------------------------------------------------------------------------------------------
# the two corpora and their models
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _corpus(devset):
    from digat_amd import synthetic
    kw, depth = synthetic.DEVSET_FIXTURES[devset]
    spec = synthetic.SynthSpec(**kw)
    return spec, synthetic.make_corpus(spec), depth


def _model(name, devset):
    from digat_amd import synthetic
    from digat_amd.model import Model, PrecomputedNewsEncoder
    spec, corpus, depth = _corpus(devset)
    state = synthetic.make_ablation_state_dict(name, spec.embedding_dim, spec.category_num, depth, seed=spec.seed + 1, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder=CHOICE[name], news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth,
                                dropout_rate=0.2)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=True)
    return model.to(_dev()).eval(), state


def _oracle_scores(name, devset, state, chunk=32):
    """fp32 CPU oracle over all rows: ``ablation_encode(..., c_n=c0)``, logits = row dot product."""
    spec, corpus, depth = _corpus(devset)
    p = O.as_params(state)
    emb = torch.from_numpy(corpus.news_embedding)
    SA = emb[torch.from_numpy(corpus.news_node_ID.astype(np.int64))]
    An_t, Mn_t = torch.from_numpy(corpus.news_graph), torch.from_numpy(corpus.news_graph_mask)
    hist = torch.from_numpy(corpus.history.astype(np.int64))
    Au_t, cm_t = torch.from_numpy(corpus.user_graph), torch.from_numpy(corpus.user_category_mask)
    ci_t = torch.from_numpy(corpus.user_category_indices)
    out = []
    with torch.no_grad():
        for s in range(0, corpus.rows, chunk):
            imp = torch.from_numpy(corpus.row_impression[s:s + chunk].astype(np.int64))
            cand = torch.from_numpy(corpus.row_candidate[s:s + chunk].astype(np.int64))
            Xn, An, Mn = SA[cand], An_t[cand], Mn_t[cand]
            c0 = Xn[:, 0] if name == "wo_SA" else O.news_graph_context(p, Xn, Mn)
            n, u = O.ablation_encode(name, p, depth, Xn, An, Mn, emb[hist[imp]], Au_t[imp], cm_t[imp], ci_t[imp], c_n=c0)
            out.append((n * u).sum(dim=1))
    return torch.cat(out).numpy()


def _repeated_candidate_rows(corpus):
    """Row index arrays of (impression, candidate) pairs that occur more than once."""
    key = corpus.row_impression.astype(np.int64) * (int(corpus.row_candidate.max()) + 1) + corpus.row_candidate.astype(np.int64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    cuts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1], True])
    return [order[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b - a > 1]


# ---------------------------------------------------------------------------------------------------------------------
# 2. the pipeline against the oracle, all five encoders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devset", ["devset_tiny", "devset_default"])
@pytest.mark.parametrize("name", list(O.ABLATIONS))
def test_ablation_pipeline_scores_ranks_metrics_match_the_oracle(name, devset):
    """util.compute_scores on the device corpus against the fp32 CPU oracle; bounds as test_hip_parity.py's pipeline test."""
    from digat_amd import evaluate, util
    spec, corpus, depth = _corpus(devset)
    model, state = _model(name, devset)
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    scores, metrics = util.compute_scores(model, dc, 256, labels=corpus.row_label)
    enc = model.graph_encoder
    if "news" in enc.GAT:
        assert tuple(dc.news_ctx_layers.shape) == (depth + 1, spec.news_num, spec.embedding_dim)
    if name == "wo_SA":
        assert float(dc.c_n0.abs().max()) == 0.0 and tuple(dc.c_n0.shape) == (spec.news_num, spec.embedding_dim)
    ref = _oracle_scores(name, devset, state)
    ref_ranks = evaluate.impression_ranks(ref, corpus.row_impression)
    ref_metrics = evaluate.scoring(corpus.row_label, ref_ranks, corpus.row_impression)
    ranks = evaluate.impression_ranks(scores, corpus.row_impression)
    err = np.abs(scores - ref)
    print(f"\n[{name}/{devset}] max|d| {err.max():.3e} (rms {np.sqrt((ref.astype(np.float64) ** 2).mean()):.3e}) "
          f"equal ranks {(ranks == ref_ranks).mean():.5f} metrics {np.round(metrics, 5)} ref {np.round(ref_metrics, 5)}")
    assert np.isfinite(scores).all()
    # a candidate that occurs twice in its impression (3.3 % / 2.6 % of the rows) must score the same bits both times: the stable
    # ranking then orders the pair as the reference does, without which the rank cap below could not hold
    repeats = _repeated_candidate_rows(corpus)
    assert repeats
    for rows in repeats:
        assert (scores[rows] == scores[rows[0]]).all(), rows
    np.testing.assert_allclose(scores, ref, rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(metrics, ref_metrics, rtol=0, atol=1e-4)
    assert (ranks == ref_ranks).mean() > 0.995


# ---------------------------------------------------------------------------------------------------------------------
# 3. grouped against per-row, all five encoders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.ABLATIONS))
def test_grouped_route_matches_the_per_row_route(name):
    """score_rows(grouped=True) against score_rows(grouped=False) on the default corpus, and ``inference_grouped`` called directly
    against ``inference`` on the expanded tensors.  The per-news table and the per-group layers are computed at other row counts
    than in-batch, so kernels chosen by row count may differ: fp32 noise, max|d| <= 2e-5 rms (test_hip_parity.py's bound for that)."""
    from digat_amd import util
    spec, corpus, depth = _corpus("devset_default")
    model, _ = _model(name, "devset_default")
    enc = model.graph_encoder
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    util.prepare_news_side(enc, dc, 256)
    calls = []
    inner = enc._grouped
    enc._grouped = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    per_row = util.score_rows(model, dc, 0, dc.rows, 256, grouped=False)
    assert not calls
    grouped = util.score_rows(model, dc, 0, dc.rows, 256, grouped=True)
    assert calls, "the grouped branch did not run"
    rms = float(per_row.double().pow(2).mean().sqrt())
    diff = float((grouped - per_row).abs().max())
    print(f"\n[{name}] score_rows grouped vs per-row: max|d| {diff:.3e}, rms {rms:.3e}")
    assert torch.isfinite(grouped).all() and diff <= 2e-5 * rms
    # ... and the encoder's own entry on one batch with 4 G <= B
    row_imp = corpus.row_impression.astype(np.int64)
    ue, Au, cm, ci, rg, Xn, An, Mn, c0 = util.gather_batch_grouped(dc, 0, dc.rows, row_imp)
    B, G = int(rg.shape[0]), int(ue.shape[0])
    assert 4 * G <= B
    del calls[:]
    with torch.no_grad():
        kw = {}
        if dc.news_ctx_layers is not None:
            kw = dict(news_ctx_layers=dc.news_ctx_layers, news_index=dc.row_candidate)
            gn, gu = enc.inference_grouped(dc.SA_news_representations, An, Mn, ue, Au, cm, ci, rg, c0, **kw)
        else:
            gn, gu = enc.inference_grouped(Xn, An, Mn, ue, Au, cm, ci, rg, c0)
        rgl = rg.long()
        pn, pu = enc.inference(Xn, An, Mn, ue.index_select(0, rgl), Au.index_select(0, rgl), cm.index_select(0, rgl),
                               ci.index_select(0, rgl), c0)
    assert len(calls) == 1
    for what, a, b in (("news", gn, pn), ("user", gu, pu)):
        scale = float(b.double().pow(2).mean().sqrt())
        dd = float((a - b).abs().max())
        print(f"[{name}] inference_grouped vs inference, {what} context: max|d| {dd:.3e}, rms {scale:.3e}")
        assert a.shape == b.shape and dd <= 2e-5 * scale, what


# ---------------------------------------------------------------------------------------------------------------------
# 4. a Trainer dev epoch with an ablation encoder
# ---------------------------------------------------------------------------------------------------------------------
def test_trainer_dev_epoch_with_an_ablation_encoder():
    from digat_amd import util
    from digat_amd.model import Model, PrecomputedNewsEncoder
    from digat_amd.trainer import SyntheticTrainSet, Trainer
    spec, corpus, depth = _corpus("devset_tiny")
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="wo_interaction", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=depth,
                                dropout_rate=0.1, epoch=1, batch_size=16, lr=1e-3, weight_decay=0.0, gradient_clip_norm=1.0)
    torch.manual_seed(0)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding), trainable=True))
    model.initialize()
    model = model.to(_dev())
    dc = util.DeviceCorpus.from_numpy(corpus, _dev())
    trainer = Trainer(model, cfg, dc, SyntheticTrainSet(corpus, 4, 0), dev_labels=corpus.row_label)
    losses = trainer.train(max_steps=2)
    assert len(losses) == 1 and np.isfinite(losses[0])
    got = (trainer.auc, trainer.mrr, trainer.ndcg5, trainer.ndcg10)
    assert all(len(m) == 1 and np.isfinite(m[0]) and 0.0 <= m[0] <= 1.0 for m in got), got
    assert trainer.best_dev_epoch == 1 and dc.news_ctx_layers is not None


# ---------------------------------------------------------------------------------------------------------------------
# 5. derived user graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_derived_user_graphs_give_the_same_scores():
    from digat_amd import util
    spec, corpus, depth = _corpus("devset_default")
    model, _ = _model("User_graph_wo_inter", "devset_default")
    table = util.DeviceCorpus.from_numpy(corpus, _dev())
    derived = util.DeviceCorpus.from_numpy(corpus, _dev(), user_graphs="derived")
    assert derived.user_graph is None and derived.user_category_mask is None
    a, _ = util.compute_scores(model, table, 256, labels=corpus.row_label)
    b, _ = util.compute_scores(model, derived, 256, labels=corpus.row_label)
    assert np.isfinite(a).all() and np.array_equal(a, b)
