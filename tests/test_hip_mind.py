"""GPU suite: the MIND loader feeding the device pipeline end to end on tests/golden/mind_tiny — user graphs and news graphs built
on the device against the reference's, dev scoring and the first training step of an MSA + DIGAT model against the reference's
(tests/golden/mind_tiny_golden.npz, minted by tools/mint_mind_golden.py), and ``main`` in-process through its four modes."""
import json
import os
import shutil
import types

import numpy as np
import pytest
import torch

from mind_common import FIXTURE, LOAD, SIMILARITY, loaded, minted

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_shared = {}


def corpus_with_graphs():
    """The fixture with its similarity file walked on the device (once)."""
    return loaded(similarity_file=SIMILARITY)


def reference_model(dropout=0.0):
    """MSA + DIGAT at the minted shapes (d = 64 as 4 x 16, word dim 20, attention 32, depth 2) with the minted state."""
    from digat_amd.model import Model
    g, corpus = minted(), corpus_with_graphs()
    c = json.loads(str(g["config"]))
    cfg = types.SimpleNamespace(news_encoder="MSA", graph_encoder="DIGAT", news_graph_size=c["news_graph_size"],
                                max_history_num=c["max_history_num"], category_num=corpus.category_num, graph_depth=c["graph_depth"],
                                dropout_rate=dropout, vocabulary_size=corpus.vocabulary_size, word_embedding_dim=c["word_embedding_dim"],
                                max_title_length=c["max_title_length"], MSA_head_num=c["MSA_head_num"], MSA_head_dim=c["MSA_head_dim"],
                                attention_dim=c["attention_dim"], epoch=1, batch_size=16, lr=1e-3, weight_decay=0.0, gradient_clip_norm=1.0)
    model = Model(cfg)
    model.initialize()
    res = model.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w_")}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(DEV), cfg


@pytest.mark.parametrize("split", ["train", "dev", "test"])
def test_user_graphs_from_indices_equal_the_references(split):
    from digat_amd import util
    s, g = loaded().splits[split], minted()
    graph, mask = util.user_graphs_from_indices(torch.from_numpy(s.user_category_indices).to(DEV), 5)
    torch.cuda.synchronize()
    assert np.array_equal(graph.cpu().numpy(), g[split + "_user_history_graph"])
    assert np.array_equal(mask.cpu().numpy(), g[split + "_user_history_category_mask"])
    # ... and the table from_numpy builds for a corpus that holds none is that graph
    dc = util.DeviceCorpus.from_numpy(corpus_with_graphs().splits[split], torch.device(DEV))
    assert dc.user_graph.dtype == torch.bool and np.array_equal(dc.user_graph.cpu().numpy(), g[split + "_user_history_graph"])
    assert np.array_equal(dc.user_category_mask.cpu().numpy(), s.user_category_mask)


def test_similarity_file_through_the_device_walk_equals_the_references_news_graphs():
    corpus, g = corpus_with_graphs(), minted()
    node_ID, graph, mask = corpus.graphs()
    assert corpus.news_graph_source == "similarity"
    assert node_ID.dtype == np.int32 and np.array_equal(node_ID, g["news_node_ID"])
    assert graph.dtype == bool and np.array_equal(graph, g["news_graph"])
    assert mask.dtype == bool and np.array_equal(mask, g["news_graph_mask"]) and not mask[:, 0].any()
    assert (mask.sum(axis=1)[1:] == 0).any() and (mask.sum(axis=1) == 3).any()      # a news with no similar news; a full graph


def dev_scores(user_graphs):
    from digat_amd import util
    if user_graphs not in _shared:
        model, _ = reference_model()
        dev = corpus_with_graphs().dev
        dc = util.DeviceCorpus.from_numpy(dev, torch.device(DEV), user_graphs=user_graphs)
        scores, metrics = util.compute_scores(model.eval(), dc, 256, labels=dev.row_label)
        _shared[user_graphs] = (scores, metrics, dc)
    return _shared[user_graphs]


def test_dev_scores_ranks_and_metrics_against_the_reference():
    """The tolerances of test_devset_pipeline_scores_ranks_metrics: scores rtol 1e-4 / atol 2e-5, metrics 1e-4."""
    from digat_amd import evaluate
    g, dev = minted(), corpus_with_graphs().dev
    scores, metrics, dc = dev_scores("table")
    err = np.abs(scores - g["dev_scores"])
    print(f"\n[mind dev] rows {len(scores)} max|diff| {err.max():.3e} (scores up to {np.abs(g['dev_scores']).max():.3f}); metrics {metrics} "
          f"reference {tuple(g['dev_metrics'])}; news representations max|diff| "
          f"{np.abs(dc.news_embedding.cpu().numpy() - g['dev_news_embedding']).max():.3e}")
    assert scores.shape == g["dev_scores"].shape and np.isfinite(scores).all()
    assert (err <= 2e-5 + 1e-4 * np.abs(g["dev_scores"])).all(), err.max()
    np.testing.assert_allclose(metrics, g["dev_metrics"], rtol=0, atol=1e-4)
    ranks = evaluate.impression_ranks(scores, dev.row_impression)
    ref_ranks = evaluate.impression_ranks(g["dev_scores"], dev.row_impression)
    assert evaluate.rank_lines(ref_ranks, dev.row_impression) == str(g["dev_rank_lines"]).split("\n")     # the reference's own rank file
    assert (ranks == ref_ranks).mean() > 0.995                                      # only near-ties may swap


def test_table_and_derived_user_graphs_score_bit_for_bit():
    table, derived = dev_scores("table"), dev_scores("derived")
    assert derived[2].user_graph is None and table[2].user_graph is not None
    assert np.array_equal(table[0], derived[0]) and table[1] == derived[1]


def test_two_splits_share_one_set_of_news_tables():
    from digat_amd import util
    corpus = corpus_with_graphs()
    model, _ = reference_model()
    a = util.DeviceCorpus.from_numpy(corpus.dev, torch.device(DEV))
    util.compute_scores(model.eval(), a, 256, labels=corpus.dev.row_label)
    b = util.DeviceCorpus.from_numpy(corpus.test, torch.device(DEV), news_from=a)
    shared = ("news_node_ID", "news_graph", "news_graph_mask", "title_text", "title_mask", "news_embedding", "SA_news_representations",
              "c_n0", "news_hpq0", "user_hpq0", "ctxq0")
    for name in shared:
        assert getattr(a, name) is not None and getattr(a, name).data_ptr() == getattr(b, name).data_ptr(), name
    before = {name: getattr(b, name).data_ptr() for name in shared}
    scores_b, _ = util.compute_scores(model, b, 256, labels=corpus.test.row_label)
    assert {name: getattr(b, name).data_ptr() for name in shared} == before       # scored from the first split's caches: nothing rebuilt
    own = util.DeviceCorpus.from_numpy(corpus.test, torch.device(DEV))
    scores_own, _ = util.compute_scores(model, own, 256, labels=corpus.test.row_label)
    assert own.c_n0.data_ptr() != a.c_n0.data_ptr() and np.array_equal(scores_b, scores_own)
    # the weights move on; the first split is scored again; the second takes its new tables over
    with torch.no_grad():
        model.graph_encoder.topic_node_embedding.add_(0.01)
    util.compute_scores(model, a, 256, labels=corpus.dev.row_label)
    assert a.c_n0.data_ptr() != before["c_n0"] or a.weights_key != b.weights_key
    moved, _ = util.compute_scores(model, b, 256, labels=corpus.test.row_label)
    assert b.c_n0.data_ptr() == a.c_n0.data_ptr() and b.weights_key == a.weights_key
    assert not np.array_equal(moved, scores_b)


def train_sets(corpus):
    """A device set after one sampling launch and a host set holding the same samples (tests/test_hip_train_input.py)."""
    from digat_amd.train_input import DeviceTrainSet
    from digat_amd.trainer import SyntheticTrainSet
    dev_set = DeviceTrainSet(corpus.train, 4, seed=7, device=DEV)
    dev_set.negative_sampling(0)
    host_set = SyntheticTrainSet(corpus.train, 4, seed=0)
    host_set.samples[:] = dev_set.samples_host()
    return host_set, dev_set


def test_three_training_steps_give_the_same_losses_through_either_input_path():
    from digat_amd import util
    from digat_amd.trainer import Trainer
    corpus = corpus_with_graphs()
    dc = util.DeviceCorpus.from_numpy(corpus.train, torch.device(DEV))

    def run(device_path):
        host_set, dev_set = train_sets(corpus)
        model, cfg = reference_model(dropout=0.1)
        trainer = Trainer(model, cfg, dc, dev_set if device_path else host_set)
        model.train()
        torch.manual_seed(123)
        losses = [trainer.train_step(idx) for k, idx in enumerate(trainer.batches(1)) if k < 3]
        assert len(losses) == 3 and all(np.isfinite(losses))
        return losses
    host, device = run(False), run(True)
    print(f"\n[mind train input] host {host}\n                   device {device}")
    assert host == device


def test_first_training_step_loss_against_the_reference():
    """The reference's loss on its first batch (dropout 0, the minted negative samples): within 1e-4 relative, the accuracy the
    reference states and this project uses as its bound."""
    from digat_amd import util
    from digat_amd.trainer import SyntheticTrainSet, Trainer, training_loss
    g, corpus = minted(), corpus_with_graphs()
    host_set = SyntheticTrainSet(corpus.train, 4, seed=0)
    assert host_set.samples.shape == g["train_samples"].shape and np.array_equal(np.array([b[1] for b in host_set.behaviors]), g["train_samples"][:, 0])
    host_set.samples[:] = g["train_samples"]
    model, cfg = reference_model(dropout=0.0)
    dc = util.DeviceCorpus.from_numpy(corpus.train, torch.device(DEV))
    trainer = Trainer(model, cfg, dc, host_set)
    model.train()
    logits = model(*trainer.gather(g["train_batch"]))
    loss = float(training_loss(logits).item())
    want = float(g["train_loss"])
    print(f"\n[mind first step] loss {loss:.8f} reference {want:.8f} relative difference {abs(loss - want) / abs(want):.3e}; "
          f"logits max|diff| {np.abs(logits.detach().cpu().numpy() - g['train_logits']).max():.3e}")
    assert abs(loss - want) <= 1e-4 * abs(want), (loss, want)


SMALL = ["--MSA_head_num", "4", "--MSA_head_dim", "16", "--cnn_kernel_num", "64", "--word_embedding_dim", "20", "--attention_dim", "32",
         "--graph_depth", "2", "--max_history_num", "10", "--max_title_length", "8", "--SAG_hops", "1", "--SAG_neighbors", "3",
         "--batch_size", "16", "--similarity_file", SIMILARITY]


@pytest.mark.parametrize("news_encoder,train_input,user_graphs", [("MSA", "host", "table"), ("CNN", "device", "derived")])
def test_main_trains_evaluates_tests_and_recommends_on_the_fixture(news_encoder, train_input, user_graphs, tmp_path, capsys):
    from digat_amd.main import main
    root, models = tmp_path / "data", tmp_path / "models"
    shutil.copytree(FIXTURE, root)
    shutil.copy(os.path.join(FIXTURE, "test_unlabelled", "behaviors.tsv"), root / "test" / "behaviors.tsv")    # MIND-large's test file
    common = ["--data_root", str(root), "--news_encoder", news_encoder, "--user_graphs", user_graphs,
              "--data_cache", str(tmp_path / "cache")] + SMALL
    name = news_encoder + "-DIGAT"
    main(["--mode", "train", "--max_steps", "4", "--model_dir", str(models), "--train_input", train_input] + common)
    out = capsys.readouterr().out
    assert "Epoch 1 : train done" in out and "AUC : " in out and os.path.exists(models / name) and os.path.exists(models / (name + "-1"))
    main(["--mode", "dev", "--dev_model_path", str(models / name)] + common)
    out = capsys.readouterr().out
    metrics = [float(line.split(" : ")[1]) for line in out.splitlines() if line.split(" : ")[0] in ("AUC", "MRR", "nDCG@5", "nDCG@10")]
    assert len(metrics) == 4 and all(np.isfinite(metrics)) and all(0.0 < m <= 1.0 for m in metrics), out
    ranks, recs = tmp_path / "ranks.txt", tmp_path / "recommend.txt"
    main(["--mode", "test", "--test_model_path", str(models / name), "--test_output_file", str(ranks)] + common)
    out = capsys.readouterr().out
    assert "AUC" not in out and "Inference time" in out             # an unlabelled split: the rank file, no metrics
    lines = ranks.read_text().split("\n")
    assert len(lines) == 24 and [int(l.split(" ")[0]) for l in lines] == list(range(1, 25))
    with open(root / "test" / "behaviors.tsv", encoding="utf-8") as f:
        sizes = [len(l.split("\t")[4].strip().split(" ")) for l in f]
    assert [sorted(json.loads(l.split(" ")[1])) for l in lines] == [list(range(1, n + 1)) for n in sizes]
    main(["--mode", "recommend", "--test_model_path", str(models / name), "--recommend_k", "5", "--recommend_output", str(recs)] + common)
    lines = recs.read_text().split("\n")
    assert len(lines) == 24 and all(len(json.loads(l.split(" ")[1])) == 5 for l in lines)
