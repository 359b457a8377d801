"""GPU suite: user graphs built on the device from category indices (digat_user_graph_build) — against the graphs the reference
minted, against the test's own loop rule over a shape sweep with guard bytes around every output, against the pinned host
restatement, and through every layer that takes ``user_graph=None`` or a corpus without the table (encoder modules, the
scoring pipeline, the trainer's gather).  Everything here is bit for bit: the outputs are bytes."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, split_fixture
from user_graph_common import RULE_FIXTURES, loop_rule, rule_fixture, scattered_indices

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-5            # the project's element-wise tolerance against golden outputs (test_hip_parity.py)
GUARD = 64
ODD_GUARD = 67                     # the byte outputs: their own base is then odd, not only the later graphs' g * U * U


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def close(got, want, what, rtol=RTOL, atol=ATOL):
    got, want = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    assert (err <= atol + rtol * np.abs(want)).all(), f"{what}: max|diff| = {err.max():.3e}"


# ---- 1. against the goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RULE_FIXTURES))
def test_kernel_reproduces_reference_minted_graphs(name):
    from digat_amd import util
    ci, C, graph, mask = rule_fixture(name)
    got_graph, got_mask, entries = util.user_graphs_from_indices(_t(ci), C, want_entries=True)
    assert got_graph.dtype == torch.bool and got_mask.dtype == torch.bool and entries.dtype == torch.int32
    assert np.array_equal(got_graph.cpu().numpy(), graph)
    assert np.array_equal(got_mask.cpu().numpy(), mask)
    assert np.array_equal(entries.cpu().numpy(), graph.reshape(len(graph), -1).sum(axis=1))


# ---- 2. shape sweep against the loop rule, guard bytes around every output ---------------------------------------------------
def _guarded(nbytes, guard=GUARD):
    """A uint8 allocation of guard + nbytes + guard (at least 64 bytes each side): guards 0xAB, payload 0xFF; (whole buffer,
    payload view)."""
    buf = torch.full((guard + nbytes + guard,), 0xAB, dtype=torch.uint8, device=_dev())
    buf[guard:guard + nbytes] = 0xFF
    return buf, buf[guard:guard + nbytes]


@pytest.mark.parametrize("with_rows", [False, True], ids=["plain", "rows"])
@pytest.mark.parametrize("H,C,G", [(1, 1, 3), (10, 5, 4), (50, 17, 33), (50, 18, 7), (111, 17, 2), (3, 125, 2)])
def test_shape_sweep_against_loop_rule(H, C, G, with_rows):
    from digat_amd import util
    rng = np.random.default_rng(1000 * H + 10 * C + G)
    U = H + C
    if with_rows:                                   # a table with more rows than graphs: permuted, one repeat, rows skipped
        table = scattered_indices(rng, G + 3, H, C)
        rows = rng.permutation(G + 3)[:G].astype(np.int64)
        rows[-1] = rows[0]
        src = table[rows]
    else:
        table, rows = scattered_indices(rng, G, H, C), None
        src = table
    want_graph, want_mask, want_entries = loop_rule(src, C)
    gbuf, gview = _guarded(G * U * U, ODD_GUARD)
    mbuf, mview = _guarded(G * (C + 1), ODD_GUARD)
    ebuf, eview = _guarded(4 * G)                   # int32: stays 4-byte aligned
    out = (gview.view(G, U, U), mview.view(G, C + 1), eview.view(torch.int32))
    got_graph, got_mask, entries = util.user_graphs_from_indices(_t(table), C, rows=None if rows is None else _t(rows), out=out,
                                                                 want_entries=True)
    torch.cuda.synchronize()
    assert got_graph.data_ptr() == gbuf.data_ptr() + ODD_GUARD and got_graph.data_ptr() % 2 == 1
    assert entries.data_ptr() == ebuf.data_ptr() + GUARD
    for what, buf, n, guard in (("graph", gbuf, G * U * U, ODD_GUARD), ("mask", mbuf, G * (C + 1), ODD_GUARD), ("entries", ebuf, 4 * G, GUARD)):
        host = buf.cpu().numpy()
        assert (host[:guard] == 0xAB).all() and (host[guard + n:] == 0xAB).all(), f"{what}: a guard byte was written"
        if what != "entries":
            assert (host[guard:guard + n] <= 1).all(), f"{what}: a byte is neither 0 nor 1"
    assert np.array_equal(got_graph.cpu().numpy(), want_graph)
    assert np.array_equal(got_mask.cpu().numpy(), want_mask)
    assert np.array_equal(entries.cpu().numpy(), want_entries)
    assert np.array_equal(entries.cpu().numpy(), got_graph.view(torch.uint8).sum(dim=(1, 2)).cpu().numpy())


# ---- 3. against the pinned host restatement -----------------------------------------------------------------------------------
def test_prefix_valid_inputs_equal_host_restatement():
    from digat_amd import synthetic, util
    H, C, G = 50, 17, 64
    rng = np.random.default_rng(5)
    hist_cat = rng.integers(0, C, size=(G, H)).astype(np.int64)
    hist_len = rng.integers(0, H + 1, size=G).astype(np.int64)
    hist_len[:3] = (0, H, 1)
    graph, mask, idx = synthetic.build_user_graphs(hist_cat, hist_len, C)
    got_graph, got_mask = util.user_graphs_from_indices(_t(idx), C)
    assert np.array_equal(got_graph.cpu().numpy(), graph) and np.array_equal(got_mask.cpu().numpy(), mask)


def test_build_is_graph_capturable():
    """include/digat_hip.h promises one launch, no allocation, no synchronisation: a build into given buffers can be captured
    into a hipGraph, and a replay reproduces the eager bytes."""
    from digat_amd import util
    H, C, G = 50, 17, 33
    ci = _t(scattered_indices(np.random.default_rng(9), G, H, C))
    eager = util.user_graphs_from_indices(ci, C, want_entries=True)
    out = tuple(torch.empty_like(t) for t in eager)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        util.user_graphs_from_indices(ci, C, out=out)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(out, eager):
        assert torch.equal(got, want)


# ---- 4. encoder modules -------------------------------------------------------------------------------------------------------
def test_encoder_derives_the_graph_when_none_is_passed():
    from digat_amd.graphEncoders import DIGAT
    fx = load_golden("tiny.npz")
    ins, w, outs = split_fixture(fx)
    B, N, H, C, d, L = (int(v) for v in fx["meta"])
    cfg = types.SimpleNamespace(news_graph_size=N, max_history_num=H, category_num=C, graph_depth=L, dropout_rate=0.2)
    enc = DIGAT(cfg, d)
    enc.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}, strict=True)
    enc = enc.to(_dev()).eval()
    b = {k: _t(v) for k, v in ins.items()}
    Xn, An, Mn, ue = b["news_graph_embeddings"], b["news_graph"], b["news_graph_mask"], b["user_news_embedding"]
    Au, cm, ci = b["user_graph"], b["user_category_mask"], b["user_category_indices"]
    with torch.no_grad():
        c_n0 = enc.compute_news_graph_context(Xn, Mn)
        given = {"forward": enc(Xn, An, Mn, ue, Au, cm, ci), "inference": enc.inference(Xn, An, Mn, ue, Au, cm, ci, c_n0)}
        derived = {"forward": enc(Xn, An, Mn, ue, None, None, ci), "inference": enc.inference(Xn, An, Mn, ue, None, None, ci, c_n0)}
    for call in ("forward", "inference"):
        for side, got, same in zip(("news", "user"), derived[call], given[call]):
            assert torch.equal(got, same), f"{call} {side}: derived graph differs from the golden graph passed in"
            close(got, outs[f"a5_{call}_{side}"], f"{call} {side} vs golden")
    with pytest.raises(ValueError):
        enc.inference(Xn, An, Mn, ue, None, cm, ci, c_n0)          # a mask without a graph: ambiguous, refused


# ---- 5. scoring pipeline, 6. trainer ------------------------------------------------------------------------------------------
def _devset_model(name):
    from digat_amd import synthetic
    from digat_amd.model import Model, PrecomputedNewsEncoder
    kw, L = synthetic.DEVSET_FIXTURES[name]
    spec = synthetic.SynthSpec(**kw)
    corpus = synthetic.make_corpus(spec)
    state = synthetic.make_state_dict(spec.embedding_dim, spec.category_num, L, seed=spec.seed + 1, bias_std=0.05)
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=spec.news_graph_size,
                                max_history_num=spec.max_history_num, category_num=spec.category_num, graph_depth=L, dropout_rate=0.2,
                                epoch=1, batch_size=16, lr=1e-3, weight_decay=0.0, gradient_clip_norm=1.0)
    model = Model(cfg, news_encoder=PrecomputedNewsEncoder(torch.from_numpy(corpus.news_embedding)))
    model.graph_encoder.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return spec, corpus, cfg, model.to(_dev()).eval()


@pytest.mark.parametrize("name", ["devset_tiny", "devset_default"])
def test_scoring_pipeline_on_a_corpus_without_the_table(name, monkeypatch):
    from digat_amd import evaluate, util
    spec, corpus, cfg, model = _devset_model(name)
    fx = load_golden(name + ".npz")
    served, built = [], []
    take, build = util.GroupedBatchPipeline.take, util.user_graphs_from_indices

    def counting_take(self, k):
        out = take(self, k)
        served.append(out is not None)
        return out

    def counting_build(cat_idx, category_num, rows=None, **kw):
        built.append(int(cat_idx.shape[0] if rows is None else rows.shape[0]))
        return build(cat_idx, category_num, rows=rows, **kw)
    monkeypatch.setattr(util.GroupedBatchPipeline, "take", counting_take)
    monkeypatch.setattr(util, "user_graphs_from_indices", counting_build)
    monkeypatch.setattr(util, "USER_GRAPH_CHUNK_ROWS", 16)      # the corpus pass (entries per node) in chunks, never one [I,U,U] build
    runs = {}
    for mode in ("table", "derived"):
        del served[:], built[:]
        dc = util.DeviceCorpus.from_numpy(corpus, _dev(), user_graphs=mode)
        assert dc.user_graph_size == spec.max_history_num + spec.category_num and dc.category_num == spec.category_num
        scores, metrics = util.compute_scores(model, dc, 256, labels=corpus.row_label)
        assert any(served), "the grouped pipeline served no batch"
        if mode == "derived":
            assert dc.user_graph is None and dc.user_category_mask is None
            # the corpus's entries per node in chunks of 16 graphs, then one build per batch: its groups (a corpus that fits one
            # batch, as these do, has all its impressions in it; a larger one never sees a build of I graphs)
            I = len(corpus.user_category_indices)
            chunks = -(-I // 16)
            assert built[:chunks] == [16] * (I // 16) + ([I % 16] if I % 16 else []) and len(built) > chunks
        else:
            assert dc.user_graph is not None and not built
        runs[mode] = (scores, metrics, evaluate.impression_ranks(scores, corpus.row_impression))
    assert np.array_equal(runs["derived"][0], runs["table"][0]), "scores differ between the derived and the table corpus"
    assert tuple(runs["derived"][1]) == tuple(runs["table"][1]) and np.array_equal(runs["derived"][2], runs["table"][2])
    scores, metrics, ranks = runs["derived"]
    close(scores, fx["scores"], "scores", rtol=1e-4, atol=2e-5)                 # test_devset_pipeline_scores_ranks_metrics' own
    np.testing.assert_allclose(metrics, fx["metrics"], rtol=0, atol=1e-4)
    assert (ranks == evaluate.impression_ranks(fx["scores"], corpus.row_impression)).mean() > 0.995


def test_per_row_gathers_on_a_corpus_without_the_table():
    """gather_batch / gather_batch_grouped (the paths a batch with too few rows per group takes)."""
    from digat_amd import util
    spec, corpus, cfg, model = _devset_model("devset_tiny")
    table = util.DeviceCorpus.from_numpy(corpus, _dev())
    derived = util.DeviceCorpus.from_numpy(corpus, _dev(), user_graphs="derived")
    for dc in (table, derived):
        util.prepare_news_side(model.graph_encoder, dc, 256)
    assert table.xattn_hint == derived.xattn_hint and "user" in derived.xattn_hint
    rows = corpus.row_impression
    for a, b in zip(util.gather_batch(table, 5, 300), util.gather_batch(derived, 5, 300)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for a, b in zip(util.gather_batch_grouped(table, 5, 300, rows), util.gather_batch_grouped(derived, 5, 300, rows)):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_trainer_gather_on_a_corpus_without_the_table():
    from digat_amd import util
    from digat_amd.trainer import SyntheticTrainSet, Trainer
    spec, corpus, cfg, model = _devset_model("devset_tiny")
    batches = {}
    for mode in ("table", "derived"):
        dc = util.DeviceCorpus.from_numpy(corpus, _dev(), user_graphs=mode)
        model.graph_encoder.corpus_xattn_hint = {}
        trainer = Trainer(model, cfg, dc, SyntheticTrainSet(corpus, 4, seed=0))
        trainer.train_set.negative_sampling()
        idx = next(iter(trainer.batches(1)))
        batches[mode] = (trainer.gather(idx), dict(model.graph_encoder.corpus_xattn_hint))
        assert (dc.user_graph is None) == (mode == "derived")
    assert batches["table"][1] == batches["derived"][1] and "user" in batches["derived"][1]
    assert len(batches["table"][0]) == len(batches["derived"][0]) == 9
    for a, b in zip(batches["table"][0], batches["derived"][0]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
